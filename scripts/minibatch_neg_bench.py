"""The captured cfg5 link step (B = 1,024 positives, the bench's model and fanouts) under four
settings of the mini-batch loss, alternating in one process, medians of 7 replays each:

  default             one uniform negative, unit weights (the reference's loss)
  k4_uniform          num_neg = 4, torch.randint draws
  k4_weighted_avoid   num_neg = 4, negatives ~ degree^0.75, seen posts redrawn
  k4_all              the same + weighting="edge" + logq = dist.log_q(4)

Per setting: ms per replayed step, the LinkSampler's prepare (GPU ms on its stream and host ms
to queue it), the recorded graph's node count, the batch's longest negatives list (the figure
that decides whether a planned dP gather for the batch is worth having) and the dP gather alone
(the loss run eagerly on the replayed step's outputs under ops.KernelTimer).

  python scripts/minibatch_neg_bench.py [--scale 1.0] [--out profiles/minibatch_neg_ab.jsonl]
"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from truth_recommendation_gnn_amd import HeteroSAGE, metrics, minibatch, ops, sampler, synth  # noqa: E402

import bench  # noqa: E402

K, REPS = 4, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default="profiles/minibatch_neg_ab.jsonl")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.CONFIGS["cfg5"] if args.scale == 1.0 else synth.scaled("cfg5", args.scale)
    g = synth.make_graph(cfg, device=dev, device_gen=True)
    rels = bench.relations_of(cfg)
    fanouts = [15, 10]
    s = sampler.NeighborSampler({"user": cfg.num_users, "post": cfg.num_posts},
                                g.edge_index_dict, [et for et, _ in rels], fanouts)
    ei = g.edge_index_dict[synth.ENGAGES]
    B, P, U = args.batch, cfg.num_posts, cfg.num_users
    order = torch.randperm(int(ei.shape[1]), device=dev,
                           generator=torch.Generator(device=dev).manual_seed(0))
    dist = ops.PostDistribution.from_degree(ei, P)
    seen = metrics.SeenIndex(ei, U, P)
    gen_w = torch.Generator(device=dev).manual_seed(3)
    w = torch.randint(0, 2, (int(ei.shape[1]),), device=dev, generator=gen_w).float() * 2 + 1
    settings = {
        "default": (1, {}, {}),
        "k4_uniform": (K, {"num_neg": K}, {}),
        "k4_weighted_avoid": (K, {"num_neg": K}, {"distribution": dist, "avoid": seen}),
        "k4_all": (K, {"num_neg": K, "weighting": "edge", "logq": dist.log_q(K)},
                   {"distribution": dist, "avoid": seen, "pos_weights": w}),
    }
    runs = {}
    for name, (k, lkw, skw) in settings.items():
        torch.manual_seed(synth.WEIGHT_SEED)
        model = HeteroSAGE(cfg.hidden, rels, num_layers=cfg.layers, in_channels=cfg.dim).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True, capturable=True)
        n_seeds = {"user": B, "post": (1 + k) * B}
        ll = minibatch.LinkLoss(B, n_seeds["user"], n_seeds["post"], dev, **lkw)
        step = minibatch.CapturedStep(model, g.x_dict, s, n_seeds, ll, opt)
        lb = minibatch.link_batch(ei, order[:B], P, torch.Generator(device=dev).manual_seed(1),
                                  k, **skw)
        lb.mb = s.sample(lb.seeds, seed=0)
        ll.load(lb.pu, lb.pp, lb.pn, lb.w, lb.seeds["post"] if "logq" in lkw else None)
        step.capture(lb.mb, warmup=2)
        runs[name] = dict(k=k, ll=ll, step=step, ls=minibatch.LinkSampler(step, ei, P, **skw),
                          gen=torch.Generator(device=dev).manual_seed(1), ms=[], prep=[],
                          host=[], longest=[], dP=[])
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for r in range(1 + REPS):                    # round 0 warms every setting up, untimed
        for name, run in runs.items():
            ids = order[(1 + r) * B:(2 + r) * B]
            e0, e1, e2 = ev(), ev(), ev()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            run["ls"].prepare(ids, 1 + r, run["gen"])
            host = (time.perf_counter() - t0) * 1e3
            e1.record()
            run["step"].step()
            e2.record()
            torch.cuda.synchronize()
            rp = run["ll"].arena.live["n_rowptr"]
            longest = int((rp[1:] - rp[:-1]).max())
            # the dP gather alone: the loss run eagerly on this step's outputs, timed per kernel
            timer = ops.KernelTimer()
            ops.set_timer(timer)
            run["ll"]({t: v for t, v in run["step"].out.items()})
            ops.set_timer(None)
            dP = sum(a["ms"] for n, a in timer.summary().items() if n.startswith("score_gather["))
            if r:
                run["prep"].append(e0.elapsed_time(e1))
                run["ms"].append(e1.elapsed_time(e2))
                run["host"].append(host)
                run["longest"].append(longest)
                run["dP"].append(dP)
    med = statistics.median
    with open(args.out, "a") as f:
        for name, run in runs.items():
            nodes = run["step"].graph_nodes()
            rec = {"setting": name, "config": cfg.name, "batch": B, "num_neg": run["k"],
                   "step_ms": round(med(run["ms"]), 4), "step_ms_all": [round(x, 4) for x in run["ms"]],
                   "prepare_gpu_ms": round(med(run["prep"]), 4),
                   "prepare_host_ms": round(med(run["host"]), 4),
                   "graph_nodes": nodes["total"], "graph_kernels": nodes["kernel"],
                   "longest_negatives_list": max(run["longest"]),
                   "longest_negatives_list_median": med(run["longest"]),
                   "dP_gather_ms": round(med(run["dP"]), 4),
                   "loss": float(run["step"].loss), "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
