"""A/B of the link loss's two kernels with the collapsed weighting and with per-edge weights
(DESIGN.md section 5): on one config's tables, U = out["user"] and P = out["post"] from a real
forward of the bench's model (bench seeds) and the weights the training step would pass,
synth.interaction_weights(num_posts)[pos[1]], alternate in one process

    A  collapsed: one device scalar mean(pos_weights)       (hgnn_edge_score_fwd_draw, ..gather2)
    B  per edge:  edge_w[p] read per position, cscale = 1   (hgnn_edge_score_fwd_w, ..gather2_w)

for the scoring pass and for the dP gather, each in the form the loss runs at this size (the dP
gather zero-packed where ops.zpack_on says so, and then unpacked as well), then once more with
bf16 rows; 7 repetitions of each after a warm-up, timed by HIP events.  Prints one JSON line per
row format: medians and min - max, the share of the kernel's algorithmic bytes that the weights
add, and `within`: whether B's median is no slower than A's by more than three times A's own
min - max spread beyond that share.

usage: python scripts/loss_weight_bench.py [--config cfg4] [--reps 7] [--out FILE]"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from truth_recommendation_gnn_amd import HeteroSAGE, ops, synth  # noqa: E402
from truth_recommendation_gnn_amd.graph import NO_SPLIT, GroupedEdges, Plan  # noqa: E402


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4),
            "max_ms": round(s[-1], 4)}


def ab(run_a, run_b, reps, extra_share):
    """Alternate A and B; B may cost `extra_share` of A plus three of A's spreads."""
    run_a()
    run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
    a, b = stats(ta), stats(tb)
    spread = a["max_ms"] - a["min_ms"]
    allowed = a["median_ms"] * extra_share + 3 * spread
    return {"collapsed": a, "per_edge": b, "delta_ms": round(b["median_ms"] - a["median_ms"], 4),
            "weights_share_of_bytes": round(extra_share, 5), "allowed_ms": round(allowed, 4),
            "within": bool(b["median_ms"] - a["median_ms"] <= allowed)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    U32, P32 = out["user"].contiguous(), out["post"].contiguous()
    marked = bool(getattr(out["user"], ops.RELU_OUT, False))
    draw = ops.draw_negatives(pos, cfg.num_posts, generator=gen)
    pre = ops.presort_negatives(cfg.num_users, cfg.num_posts, pos, draw, "user")
    csr = ops.relation_csr_for_loss(pos, cfg.num_users, cfg.num_posts)
    by_post = GroupedEdges(pre.rowptr, pre.users, pre.users, Plan(NO_SPLIT, 0, 0, None, None),
                           cfg.num_posts)
    negs = ops._Negatives.of(draw, csr.num_edges, cfg.num_posts)
    ew = ops.edge_weights_in_kernel_order(csr, pw)
    E, nu, np_, d = csr.num_edges, cfg.num_users, cfg.num_posts, int(U32.shape[1])
    inv_e = 1.0 / E
    del g, model, out
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"setup {time.time() - t0:.1f}s  U {tuple(U32.shape)}  E={E}", file=sys.stderr,
          flush=True)
    dP = torch.empty_like(P32)

    for rows in ("fp32", "bf16"):
        if rows == "bf16":
            if d % 8:
                continue
            U, P = ops.rows_to_bf16(U32), ops.rows_to_bf16(P32)
        else:
            U, P = U32, P32
        rb = d * U.element_size()
        score_bytes = E * (2 * rb + 12) + nu * (rb + 4 * d)
        gather_bytes = 2 * E * (rb + 4) + np_ * (rb + 4 * d)
        line = {"what": "link loss kernels: collapsed weighting vs per-edge weights",
                "config": cfg.name, "rows": rows, "n_users": nu, "n_posts": np_, "d": d,
                "edges_pos": E, "weights_mean": round(float(c), 6),
                "weights_distinct": sorted(set(torch.unique(pw).cpu().tolist()))}
        line["scoring_pass"] = ab(
            lambda: ops._loss_scoring_pass(U, P, csr, negs, c, E, None),
            lambda: ops._loss_scoring_pass(U, P, csr, negs, ew.one, E, None, ew.by_user),
            args.reps, 4 * E / score_bytes)
        Uz = ops.zpack_rows(U) if rows == "fp32" and ops.zpack_on(U, marked) else None
        forms = [("dP_gather_zero_packed", Uz)] if Uz is not None else []
        forms.append(("dP_gather", None))
        for name, z in forms:
            line[name] = ab(
                lambda: ops._score_gather2(U, P, csr.fwd, by_post, c, inv_e, dP, z),
                lambda: ops._score_gather2(U, P, csr.fwd, by_post, ew.one, inv_e, dP, z,
                                           ew.by_post),
                args.reps, 4 * E / gather_bytes)
        del Uz
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
