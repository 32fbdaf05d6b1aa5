"""The sampled-softmax link loss against the BCE link loss on the same negatives (DESIGN.md
section 5), measured: on one config's tables, U = out["user"] and P = out["post"] from a real
forward of the bench's model (bench seeds), with SkewedNegatives drawn in proportion to
degree^0.75 (ops.PostDistribution.from_degree), the timed passes of the two losses

    pass            softmax (ops._edge_softmax)         BCE (ops._edge_bce)
    scoring_pass    edge_softmax_d{d}                   edge_score_d{d}
    sort            sort_negatives_coef                 sort_negatives
    plan            plan_negatives                      plan_negatives
    gather          coef_gather_planned[...]            score_gather_planned[...]

for k in --ks (default 1, 4) on fp32 and on bf16 rows.  The two losses and the settings alternate
in one process, --reps repetitions of each after a warm-up; every pass is timed by the
ops.KernelTimer's own HIP events inside the loss call.  One JSON line per setting: per pass and
loss the median and min - max, the timer's algorithmic bytes, the achieved TB/s on them, and the
softmax pass's ratio to the BCE pass (median over median).

Run it under a time limit of its own, e.g. `timeout -k 10 900 python scripts/...`.

usage: python scripts/softmax_loss_bench.py [--config cfg4] [--ks 1,4] [--reps 7]
                                            [--temperature 0.2] [--out FILE]"""
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


def timed(fn):
    """One loss call under a KernelTimer: {pass name: (ms, bytes)}."""
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        fn()
    finally:
        ops.set_timer(None)
    return {name: (v["ms"], v["bytes"]) for name, v in timer.summary().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--ks", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--temperature", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
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
    dist = ops.PostDistribution.from_degree(pos, cfg.num_posts, power=0.75)
    negs = {k: ops.sample_negatives(pos, cfg.num_posts, gen, num_neg=k, distribution=dist)
            for k in ks}
    logq = {k: ops.logq_table(csr, dist.log_q(k)) for k in ks}
    del g, model, out, pw
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"setup {time.time() - t0:.1f}s  U {tuple(U32.shape)}  E={E}", file=sys.stderr,
          flush=True)
    names = {
        "softmax": {"scoring_pass": f"edge_softmax_d{d}", "sort": "sort_negatives_coef",
                    "plan": "plan_negatives", "gather": f"coef_gather_planned[{np_}<-{nu}]x{d}"},
        "bce": {"scoring_pass": f"edge_score_d{d}", "sort": "sort_negatives",
                "plan": "plan_negatives", "gather": f"score_gather_planned[{np_}<-{nu}]x{d}"},
    }
    tables = {"fp32": (U32, P32)}
    if d % 8 == 0:
        bu = ops.rows_to_bf16(U32)
        tables["bf16"] = (bu, ops.rows_to_bf16(P32))
    tau = float(args.temperature)

    def run(loss, rows, k):
        U, P = tables[rows]
        if loss == "softmax":
            # (check=True, the entry points' default: the sort then makes no validation pass
            # over the keys, as BCE's makes none; its one host sync comes after the last launch)
            return timed(lambda: ops._edge_softmax(U, P, csr, negs[k], c, True, None, logq[k],
                                                   tau))
        return timed(lambda: ops._edge_bce(U, P, csr, negs[k], c, False, E, logq=logq[k]))

    settings = [(rows, k) for rows in tables for k in ks]
    for s in settings:                                     # warm-up (and the cached payloads)
        for loss in ("bce", "softmax"):
            run(loss, *s)
    torch.cuda.synchronize()
    runs = {(loss, s): [] for s in settings for loss in names}
    for _ in range(args.reps):
        for s in settings:                                 # settings and losses alternate
            for loss in ("bce", "softmax"):
                runs[(loss, s)].append(run(loss, *s))
    for rows, k in settings:
        line = {"what": "sampled-softmax link loss against the BCE link loss, same negatives",
                "config": cfg.name, "rows": rows, "k": k, "temperature": tau, "logq": True,
                "negatives": "SkewedNegatives, degree^0.75", "n_users": nu, "n_posts": np_,
                "d": d, "edges_pos": E, "reps": args.reps,
                "zero_packed_gather": any(n.startswith("zpack[")
                                          for n in runs[("softmax", (rows, k))][0])}
        for loss in names:
            rs = runs[(loss, (rows, k))]
            line[loss] = {}
            for key, name in names[loss].items():
                st = stats([r[name][0] for r in rs])
                st["bytes"] = rs[0][name][1]
                st["TBps"] = round(st["bytes"] / st["median_ms"] / 1e9, 3)
                line[loss][key] = st
            zp = [n for n in rs[0] if n.startswith("zpack[")]
            if zp:
                line[loss]["zpack"] = stats([r[zp[0]][0] for r in rs])
            line[loss]["total_ms"] = round(sum(v["median_ms"] for v in line[loss].values()), 4)
        line["ratio"] = {key: round(line["softmax"][key]["median_ms"]
                                    / line["bce"][key]["median_ms"], 4) for key in names["bce"]}
        line["ratio"]["total"] = round(line["softmax"]["total_ms"] / line["bce"]["total_ms"], 4)
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
