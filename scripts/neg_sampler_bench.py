"""Popularity-weighted negatives, measured on one config's graph and on
U = out["user"], P = out["post"] from a real forward of the bench's model (bench seeds):

    draw_uniform        ops.sample_negatives(...)                      hgnn_uniform_i32
    draw_weighted       ... distribution=PostDistribution.from_degree  hgnn_weighted_i32
    draw_weighted_avoid ... and avoid=SeenIndex(positives)             hgnn_weighted_avoid_i32
                        (with the share of draws that kept a seen post after max_tries)
    sort_negatives      the (post, user) pairs grouped by post, for the uniform and for the
                        weighted negatives (hgnn_sort_pairs_i32)
    plan_negatives      the device-side plan of the weighted negatives' lists (hgnn_plan_device)
    dP_gather           hgnn_score_gather2* on the uniform negatives against
                        hgnn_score_gather2_planned on the weighted ones

The settings alternate in one process, --reps repetitions of each after a warm-up.  The draws are
timed with HIP events around the call, the loss's passes by the ops.KernelTimer's own events
inside the loss call.  One JSON line per quantity: median and min - max, the bytes it moves (a
draw: 4 B written per draw, with avoid 4 B of user id read per draw too; the tables it searches
stay in the caches) and the achieved GB/s.  The unplanned gather is not run on the weighted
negatives: its longest list is summed by one wave.

Run it under a time limit of its own, e.g. `timeout -k 10 900 python scripts/...`.

usage: python scripts/neg_sampler_bench.py [--config cfg4] [--k 1] [--reps 7] [--out FILE]"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from truth_recommendation_gnn_amd import HeteroSAGE, SeenIndex, ops, synth  # noqa: E402


def stats(ts, nbytes):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "bytes": int(nbytes), "GBps": round(nbytes / med / 1e6, 1)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return res, a.elapsed_time(b)


def dP_passes(U, P, csr, neg, c, E):
    """The loss's dP chain under a KernelTimer: {pass name: (ms, bytes)}."""
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        ops._edge_bce(U, P, csr, neg, c, False, E)
    finally:
        ops.set_timer(None)
    return {name: (v["ms"], v["bytes"]) for name, v in timer.summary().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-tries", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    cfg = synth.CONFIGS[args.config]
    k = args.k
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
    U, P = out["user"].contiguous(), out["post"].contiguous()
    setattr(U, ops.RELU_OUT, marked)
    csr = ops.relation_csr_for_loss(pos, cfg.num_users, cfg.num_posts)
    E, nu, np_, d = csr.num_edges, cfg.num_users, cfg.num_posts, int(U.shape[1])
    n = E * k
    dist = ops.PostDistribution.from_degree(pos, np_)
    seen = SeenIndex(pos, nu, np_)
    del g, model, out, pw
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    deg = (csr.fwd.rowptr[1:] - csr.fwd.rowptr[:-1]).double()
    p_max = float(dist.q.max()) / dist.T
    print(f"setup {time.time() - t0:.1f}s  U {tuple(U.shape)}  E={E}  chunk={csr.fwd.plan.chunk}  "
          f"max degree {int(deg.max())}  p_max {p_max:.5f}", file=sys.stderr, flush=True)
    kept = torch.zeros(1, dtype=torch.int64, device=dev)

    draws = {
        "draw_uniform": (lambda: ops.sample_negatives(pos, np_, gen, num_neg=k), 4 * n),
        "draw_weighted": (lambda: ops.sample_negatives(pos, np_, gen, num_neg=k,
                                                       distribution=dist), 4 * n),
        "draw_weighted_avoid": (lambda: ops.sample_negatives(
            pos, np_, gen, num_neg=k, distribution=dist, avoid=seen, max_tries=args.max_tries,
            kept_seen=kept), 8 * n),
    }
    neg_u = ops.sample_negatives(pos, np_, gen, num_neg=k)
    neg_w = ops.sample_negatives(pos, np_, gen, num_neg=k, distribution=dist)
    lens = torch.bincount(neg_w.values.reshape(-1).long(), minlength=np_)
    longest_w, heavy_w = int(lens.max()), int((lens > csr.fwd.plan.chunk).sum())
    longest_u = int(torch.bincount(neg_u.reshape(-1).long(), minlength=np_).max())
    del lens
    for fn, _ in draws.values():                            # warm-up
        fn()
    dP_passes(U, P, csr, neg_u, c, E)
    dP_passes(U, P, csr, neg_w, c, E)
    torch.cuda.synchronize()
    kept.zero_()
    t_draw = {name: [] for name in draws}
    runs = {"uniform": [], "weighted": []}
    for _ in range(args.reps):                              # the settings alternate
        for name, (fn, _) in draws.items():
            t_draw[name].append(timed(fn)[1])
        runs["uniform"].append(dP_passes(U, P, csr, neg_u, c, E))
        runs["weighted"].append(dP_passes(U, P, csr, neg_w, c, E))
    kept_share = int(kept) / (args.reps * n)
    head = {"what": "popularity-weighted negatives", "config": cfg.name, "k": k, "n_users": nu,
            "n_posts": np_, "d": d, "edges_pos": E, "draws": n, "reps": args.reps}
    lines = []
    for name, (_, nbytes) in draws.items():
        line = dict(head, quantity=name, **stats(t_draw[name], nbytes))
        if name == "draw_weighted_avoid":
            line["max_tries"] = args.max_tries
            line["kept_seen_share"] = round(kept_share, 6)
        lines.append(line)
    gathers = {"uniform": f"score_gather[{np_}<-{nu}]x{d}",
               "weighted": f"score_gather_planned[{np_}<-{nu}]x{d}"}
    for kind in ("uniform", "weighted"):
        first = runs[kind][0]
        names = [("sort_negatives", "sort_negatives"), ("dP_gather", gathers[kind])]
        if kind == "weighted":
            names.insert(1, ("plan_negatives", "plan_negatives"))
        for quantity, name in names:
            line = dict(head, quantity=quantity, negatives=kind, pass_name=name,
                        **stats([r[name][0] for r in runs[kind]], first[name][1]))
            if quantity == "dP_gather":
                line["zero_packed_gather"] = any(x.startswith("zpack[") for x in first)
                line["longest_list"] = longest_w if kind == "weighted" else longest_u
                if kind == "weighted":
                    line["heavy_lists"] = heavy_w
                    line["chunk"] = csr.fwd.plan.chunk
                    line["neg_slab_bytes"] = 2 * (n // csr.fwd.plan.chunk) * d * 4
            lines.append(line)
    for line in lines:
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
