"""Gate measurement of the zero-packed dP gather: on one config's tables, with
U = out["user"] and P = out["post"] taken from a real forward of the bench's model (bench seeds;
random data would have no zeros), alternate in one process

    A  the unpacked dP gather (hgnn_score_gather2)
    B  the pack pass + the packed dP gather (hgnn_zpack_rows + hgnn_score_gather2_zp)

7 repetitions of each after a warm-up, timed by HIP events; B's two launches are also timed
apart.  Prints one JSON line: the medians and min - max of each, the zero fraction of U, the
lines-per-row histogram the pack pass fills, whether the two dP are bitwise equal, and the
verdict of the gate (B faster than A by more than three times A's min - max spread).

usage: python scripts/zpack_bench.py [--config cfg4] [--reps 7] [--once] [--out FILE]
  --once: one launch of each kernel after the setup and no timing (for a counter-only profiler
          pass, e.g. rocprofv3 --pmc FETCH_SIZE -- python scripts/zpack_bench.py --once)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
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
    U, P = out["user"].contiguous(), out["post"].contiguous()
    marked = bool(getattr(out["user"], ops.RELU_OUT, False))
    neg = ops.draw_negatives(pos, cfg.num_posts, generator=gen)
    pre = ops.presort_negatives(cfg.num_users, cfg.num_posts, pos, neg, "user")
    csr = ops.relation_csr_for_loss(pos, cfg.num_users, cfg.num_posts)
    negs = GroupedEdges(pre.rowptr, pre.users, pre.users, Plan(NO_SPLIT, 0, 0, None, None),
                        cfg.num_posts)
    E = csr.num_edges
    inv_e = 1.0 / E
    del g, model, out
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"setup {time.time() - t0:.1f}s  U {tuple(U.shape)}  E={E}", file=sys.stderr, flush=True)

    dA = torch.empty_like(P)
    dB = torch.empty_like(P)
    hist = torch.zeros(6, dtype=torch.int64, device=dev)
    Uz = ops.zpack_rows(U, hist)                      # (also the warm-up of the pack pass)
    hist = hist.cpu().tolist()

    def run_a():
        ops._score_gather2(U, P, csr.fwd, negs, c, inv_e, dA)

    def run_pack():
        nonlocal Uz
        Uz = None
        Uz = ops.zpack_rows(U)

    def run_zp():
        ops._score_gather2(U, P, csr.fwd, negs, c, inv_e, dB, Uz)

    def run_b():
        run_pack()
        run_zp()

    if args.once:
        run_a()
        run_b()
        torch.cuda.synchronize()
        return
    run_a()
    run_b()
    torch.cuda.synchronize()
    equal = bool(torch.equal(dA, dB))
    ta, tb, tp, tz = [], [], [], []
    for _ in range(args.reps):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        tp.append(timed(run_pack))
        tz.append(timed(run_zp))
    a, b = stats(ta), stats(tb)
    spread = a["max_ms"] - a["min_ms"]
    n = U.shape[0]
    lines = sum(i * h for i, h in enumerate(hist)) / n
    line = {
        "what": "zpack gate: unpacked dP gather vs pack + packed dP gather", "config": cfg.name,
        "n_users": n, "n_posts": int(P.shape[0]), "d": int(U.shape[1]), "edges_pos_neg": 2 * E,
        "relu_marked": marked, "zero_fraction_U": round(float((U == 0).float().mean()), 4),
        "lines_per_row_hist": hist, "lines_per_row_mean": round(lines, 4),
        "unpacked_gather": a, "pack_plus_packed_gather": b, "pack": stats(tp),
        "packed_gather": stats(tz), "dP_bitwise_equal": equal,
        "gain_ms": round(a["median_ms"] - b["median_ms"], 4), "spread_unpacked_ms": round(spread, 4),
        "gate_passed": bool(equal and a["median_ms"] - b["median_ms"] > 3 * spread),
    }
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
