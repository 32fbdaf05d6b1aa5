"""Hard-negative mining (ops.mine_hard_negatives), measured at one config's
scale: U = out["user"] and P = out["post"] from a real forward of the bench's model (bench seeds),
the positive edges of the config's graph (Zipf posts), and per positive edge a pool of M candidates

    uniform_seed      a NegativeDraw: the pool is drawn inside the kernel
    uniform_tensor    the same draws materialised (NegativeDraw.tensor()) and read as ids
    weighted          posts in proportion to degree^0.75 (sample_negatives with a PostDistribution)

for M in --ms (default 4, 8), k = 1 and 2, on fp32 and on bf16 rows.

Yardstick: the existing k-negative scoring pass (hgnn_edge_score_fwd_k / _k_bf16) at k = M - 1 on
negatives of the same kind, which reads the same M post rows per edge (the positive and M - 1
negatives) and does more per row (exp, the dU fma).  The three calls of a setting alternate in one
process, --reps repetitions of each after a warm-up, every call timed by the ops.KernelTimer's own
HIP events.  One JSON line per setting: medians and min - max, TB/s on the timer's algorithmic
bytes, and ratio = mining (k = 2) / scoring pass, with both spreads beside it.

Run it under a time limit of its own, e.g. `timeout -k 10 900 python scripts/...`.

usage: python scripts/hard_neg_bench.py [--config cfg4] [--ms 4,8] [--reps 7] [--out FILE]"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from truth_recommendation_gnn_amd import HeteroSAGE, ops, synth  # noqa: E402


def stats(recs):
    s = sorted(ms for ms, _ in recs)
    med = s[len(s) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "spread": round((s[-1] - s[0]) / med, 4), "bytes": recs[0][1],
            "TBps": round(recs[0][1] / med / 1e9, 3)}


def timed(name, fn):
    """One call under a KernelTimer: (ms, bytes) of the pass called ``name``."""
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        fn()
    finally:
        ops.set_timer(None)
    v = timer.summary()[name]
    return v["ms"], v["bytes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--ms", default="4,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ms = [int(m) for m in args.ms.split(",")]
    if min(ms) < 3:
        raise SystemExit("--ms: M >= 3, so that k = 2 fits and the yardstick has k = M - 1 >= 2")
    dev = torch.device("cuda")
    cfg = synth.CONFIGS[args.config]
    t0 = time.time()
    torch.manual_seed(synth.WEIGHT_SEED)
    gen = torch.Generator(device=dev).manual_seed(synth.NEG_SEED)
    g = synth.make_graph(cfg, device=dev, device_gen=True)
    pos = g.edge_index_dict[synth.ENGAGES]
    model = HeteroSAGE(cfg.hidden, bench.relations_of(cfg), num_layers=cfg.layers,
                       in_channels=cfg.dim).to(dev)
    with torch.no_grad():
        out = model(g.x_dict, g.edge_index_dict)
    U32, P32 = out["user"].detach().contiguous(), out["post"].detach().contiguous()
    csr = ops.relation_csr_for_loss(pos, cfg.num_users, cfg.num_posts)
    E, nu, np_, d = csr.num_edges, cfg.num_users, cfg.num_posts, int(U32.shape[1])
    dist = ops.PostDistribution.from_degree(pos, np_, 0.75)
    c = torch.ones((), device=dev)
    del g, model, out
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"setup {time.time() - t0:.1f}s  U {tuple(U32.shape)}  E={E}", file=sys.stderr,
          flush=True)
    tables = {"fp32": (U32, P32)}
    if d % 8 == 0:
        tables["bf16"] = (ops.rows_to_bf16(U32), ops.rows_to_bf16(P32))
    score = f"edge_score_d{d}"
    for M in ms:
        draw = ops.draw_negatives(pos, np_, gen, num_neg=M)
        pools = {"uniform_seed": draw, "uniform_tensor": draw.tensor(),
                 "weighted": ops.sample_negatives(pos, np_, gen, num_neg=M, distribution=dist)}
        # the yardstick's negatives, of the same kind: M - 1 per edge
        draw_y = ops.draw_negatives(pos, np_, gen, num_neg=M - 1)
        yard = {"uniform_seed": draw_y, "uniform_tensor": draw_y.tensor(),
                "weighted": ops.sample_negatives(pos, np_, gen, num_neg=M - 1,
                                                 distribution=dist).values}
        for rows, (U, P) in tables.items():
            for pool, cand in pools.items():
                negs = ops._Negatives.of(yard[pool], E, np_)
                calls = {
                    "mine_k1": ("hard_negatives", lambda: ops.mine_hard_negatives(
                        U, P, pos, cand, num_neg=1)),
                    "mine_k2": ("hard_negatives", lambda: ops.mine_hard_negatives(
                        U, P, pos, cand, num_neg=2)),
                    "scoring_pass": (score, lambda: ops._loss_scoring_pass(
                        U, P, csr, negs, c, E * (M - 1), None)),
                }
                for name, fn in calls.values():            # warm-up
                    timed(name, fn)
                runs = {key: [] for key in calls}
                for _ in range(args.reps):
                    for key, (name, fn) in calls.items():  # the calls alternate
                        runs[key].append(timed(name, fn))
                line = {"what": "hard-negative mining against the k-negative scoring pass at "
                                "k = M - 1 (the same M post rows per edge)",
                        "config": cfg.name, "rows": rows, "M": M, "pool": pool, "n_users": nu,
                        "n_posts": np_, "d": d, "edges_pos": E, "reps": args.reps,
                        "scoring_pass_k": M - 1}
                for key in calls:
                    line[key] = stats(runs[key])
                line["ratio_k2_vs_scoring_pass"] = round(
                    line["mine_k2"]["median_ms"] / line["scoring_pass"]["median_ms"], 4)
                s = json.dumps(line)
                print(s, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(s + "\n")
        del pools, yard, draw, draw_y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
