"""The link loss with k negatives per positive edge, measured: on one
config's tables, U = out["user"] and P = out["post"] from a real forward of the bench's model
(bench seeds), the loss's three timed passes

    sort_negatives          the E k (post, user) pairs grouped by post (hgnn_draw_sort_negatives)
    score_gather[...]       dP: both lists in one gather (hgnn_score_gather2*, zero-packed where
                            ops.zpack_on says so, as the loss runs it)
    edge_score_d{d}         loss + dU: k = 1 is the one-negative kernel (hgnn_edge_score_fwd_draw /
                            _bf16, unchanged code), k >= 2 hgnn_edge_score_fwd_k / _k_bf16

for k in --ks (default 1, 2, 4) on fp32 and on bf16 rows.  The settings alternate in one process,
--reps repetitions of each after a warm-up; every pass is timed by the ops.KernelTimer's own HIP
events inside the loss call, so the times and the bytes are those of bench.py's breakdown.  One
JSON line per setting: medians and min - max, the achieved GB/s on the timer's bytes, and for the
scoring pass of k >= 2 the two yardsticks from the k = 1 pass of the same run:

    k_calls_ms      k times the one-negative pass: what k separate calls would cost
    byte_model_ms   the one-negative pass's achieved byte rate applied to this pass's bytes
                    ((1 + k) rows instead of 2 per edge)

Run it under a time limit of its own, e.g. `timeout -k 10 900 python scripts/...`.

usage: python scripts/loss_multi_neg_bench.py [--config cfg4] [--ks 1,2,4] [--reps 7]
                                              [--out FILE]"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from truth_recommendation_gnn_amd import HeteroSAGE, ops, synth  # noqa: E402


def stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4),
            "max_ms": round(s[-1], 4)}


def one_loss(U, P, csr, draw, c, E):
    """One loss call under a KernelTimer: {pass name: (ms, bytes)}."""
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        ops._edge_bce(U, P, csr, draw, c, False, E)
    finally:
        ops.set_timer(None)
    return {name: (v["ms"], v["bytes"]) for name, v in timer.summary().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--ks", default="1,2,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    if 1 not in ks:
        raise SystemExit("--ks must hold 1: the one-negative pass is the yardstick")
    dev = torch.device("cuda")
    cfg = synth.CONFIGS[args.config]
    t0 = time.time()
    torch.manual_seed(synth.WEIGHT_SEED)
    gen = torch.Generator(device=dev).manual_seed(synth.NEG_SEED)
    g = synth.make_graph(cfg, device=dev, device_gen=True)
    pos = g.edge_index_dict[synth.ENGAGES]
    pw = synth.interaction_weights(cfg.num_posts).to(dev)[pos[1]]
    c = pw.mean().to(torch.float32).reshape(()).contiguous()
    model = HeteroSAGE(cfg.hidden, bench.relations_of(cfg), num_layers=cfg.layers,
                       in_channels=cfg.dim).to(dev)
    with torch.no_grad():
        out = model(g.x_dict, g.edge_index_dict)
    marked = bool(getattr(out["user"], ops.RELU_OUT, False))
    U32, P32 = out["user"].contiguous(), out["post"].contiguous()
    setattr(U32, ops.RELU_OUT, marked)
    csr = ops.relation_csr_for_loss(pos, cfg.num_users, cfg.num_posts)
    E, nu, np_, d = csr.num_edges, cfg.num_users, cfg.num_posts, int(U32.shape[1])
    draws = {k: ops.draw_negatives(pos, cfg.num_posts, generator=gen, num_neg=k) for k in ks}
    del g, model, out, pw
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"setup {time.time() - t0:.1f}s  U {tuple(U32.shape)}  E={E}", file=sys.stderr,
          flush=True)
    score, gather = f"edge_score_d{d}", f"score_gather[{np_}<-{nu}]x{d}"
    tables = {"fp32": (U32, P32)}
    if d % 8 == 0:
        tables["bf16"] = (ops.rows_to_bf16(U32), ops.rows_to_bf16(P32))
    settings = [(rows, k) for rows in tables for k in ks]
    for rows, k in settings:                               # warm-up (and the cached payloads)
        one_loss(*tables[rows], csr, draws[k], c, E)
    torch.cuda.synchronize()
    runs = {s: [] for s in settings}
    for _ in range(args.reps):
        for s in settings:                                 # the settings alternate
            runs[s].append(one_loss(*tables[s[0]], csr, draws[s[1]], c, E))
    lines = {}
    for rows, k in settings:
        line = {"what": "link loss passes with k negatives per positive edge",
                "config": cfg.name, "rows": rows, "k": k, "n_users": nu, "n_posts": np_, "d": d,
                "edges_pos": E, "reps": args.reps,
                "zero_packed_gather": any(n.startswith("zpack[") for n in runs[(rows, k)][0])}
        for key, name in (("scoring_pass", score), ("sort_negatives", "sort_negatives"),
                          ("dP_gather", gather)):
            st = stats([r[name][0] for r in runs[(rows, k)]])
            st["bytes"] = runs[(rows, k)][0][name][1]
            st["GBps"] = round(st["bytes"] / st["median_ms"] / 1e6, 1)
            line[key] = st
        lines[(rows, k)] = line
    for rows, k in settings:
        line, base = lines[(rows, k)], lines[(rows, 1)]["scoring_pass"]
        if k > 1:
            sp = line["scoring_pass"]
            sp["k_calls_ms"] = round(k * base["median_ms"], 4)
            sp["byte_model_ms"] = round(base["median_ms"] * sp["bytes"] / base["bytes"], 4)
            sp["vs_k_calls"] = round(sp["median_ms"] / sp["k_calls_ms"], 4)
            sp["vs_byte_model"] = round(sp["median_ms"] / sp["byte_model_ms"], 4)
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
