#!/usr/bin/env python3
"""Serving at cfg2 scale: ``recommend(..., users=, exclude=)`` over the cfg2 feature tables (d=64;
--dim 128 pads them with fresh columns), the exclusion lists being cfg2's engages edges.

Two user subsets: (a) 100,000 seeded random users, (b) the 128 users with the most seen posts,
the worst case for the kernel's walk over the lists.  For each, in one process and alternating
within every repetition (one warm-up, then the median of --reps): the fused kernel alone with HIP
events, plain (hgnn_score_topk / _bf16 with ``rows``) and excluding (hgnn_score_topk_excl / _bf16),
and the whole ``recommend`` call with and without ``exclude``.  One JSON line per subset.

--ref-lib NAME (repeatable) adds the plain and the excluding kernel of another build of the
library, a file under the package's lib/ (e.g. the parent commit's build copied there as
libhgnn_parent.so), to the same alternating loop; giving the same build under two names measures
the run-to-run spread.
python scripts/recommend_bench.py [--dim 64|128] [--row-dtype fp32|bf16] [--ref-lib NAME ...]"""
import argparse
import ctypes
import json
import os
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from truth_recommendation_gnn_amd import _native as N, metrics, ops, synth  # noqa: E402

K = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--row-dtype", choices=ops.ROW_DTYPES, default="fp32")
    ap.add_argument("--ref-lib", action="append", default=[])
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5")
    bf16 = args.row_dtype == "bf16"
    dev = torch.device("cuda")
    cfg = synth.CONFIGS["cfg2"]
    g = synth.make_graph(cfg, device=dev)
    U, P = g.x_dict["user"], g.x_dict["post"]
    if args.dim != U.shape[1]:
        gen = torch.Generator(device=dev).manual_seed(7)
        extra = args.dim - U.shape[1]
        U = torch.cat([U, torch.randn(U.shape[0], extra, device=dev, generator=gen) * 0.1], 1)
        P = torch.cat([P, torch.randn(P.shape[0], extra, device=dev, generator=gen) * 0.1], 1)
    U, P = U.contiguous(), P.contiguous()
    n_u, C = int(U.shape[0]), int(P.shape[0])
    seen = metrics.SeenIndex(g.edge_index_dict[synth.ENGAGES], n_u, C)
    degree = (seen.rowptr[1:] - seen.rowptr[:-1]).long()
    gen = torch.Generator(device=dev).manual_seed(11)
    subsets = {"random_100k": torch.randperm(n_u, device=dev, generator=gen)[:100_000],
               "top128_by_seen": torch.topk(degree, 128).indices}
    entry = "hgnn_score_topk" + ("_bf16" if bf16 else "")
    entry_x = entry.replace("topk", "topk_excl")
    libs = {"this": N.lib()}
    for name in args.ref_lib:
        ref = ctypes.CDLL(str(N.LIB_PATH.parent / pathlib.Path(name).name))
        for e in (entry, entry_x):
            getattr(ref, e).restype, getattr(ref, e).argtypes = N._SIGS[e]
        libs[name] = ref
    Pk = ops.rows_to_bf16(P) if bf16 else P
    st = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for label, users in subsets.items():
        n = int(users.numel())
        users32 = users.to(torch.int32).contiguous()
        # the kernel's inputs as recommend passes them: bf16 casts the selected rows only
        Uk, rows = (ops.rows_to_bf16(U.index_select(0, users)), None) if bf16 else (U, users32)
        topv = torch.empty(n, K, device=dev)
        topi = torch.empty(n, K, dtype=torch.int32, device=dev)
        head = (N.ptr(Uk), N.ptr(rows), n, N.ptr(Pk), C, args.dim, K)
        tail = (N.ptr(topv), N.ptr(topi), N.stream_ptr(dev))
        excl = (N.ptr(seen.rowptr), N.ptr(seen.col), N.ptr(users32))
        launches = {}
        for name, lib in libs.items():
            launches[f"plain[{name}]"] = (getattr(lib, entry), head + tail)
            launches[f"excl[{name}]"] = (getattr(lib, entry_x), head + excl + tail)
        calls = {"recommend": lambda: metrics.recommend(U, P, K, users=users,
                                                        row_dtype=args.row_dtype),
                 "recommend_exclude": lambda: metrics.recommend(U, P, K, users=users, exclude=seen,
                                                                row_dtype=args.row_dtype)}
        k_ms = {name: [] for name in launches}
        c_ms = {name: [] for name in calls}
        order = list(launches.items())
        for rep in range(args.reps + 1):
            order = order[1:] + order[:1]   # every launch takes every place in the round
            for name, (fn, a) in order:
                ev[0].record(st)
                N.check(fn(*a), name)
                ev[1].record(st)
                torch.cuda.synchronize()
                k_ms[name].append(ev[0].elapsed_time(ev[1]))
            for name, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                c_ms[name].append((time.perf_counter() - t0) * 1e3)
        res = {"subset": label, "users": n, "posts": C, "dim": args.dim,
               "row_dtype": args.row_dtype, "K": K, "reps": args.reps,
               "seen_posts": int(degree[users].sum()), "max_seen": int(degree[users].max()),
               "kernel_ms": {name: round(statistics.median(v[1:]), 4) for name, v in k_ms.items()},
               "kernel_ms_min_max": {name: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
                                     for name, v in k_ms.items()},
               "call_ms": {name: round(statistics.median(v[1:]), 3) for name, v in c_ms.items()}}
        res["excl_over_plain"] = round(res["kernel_ms"]["excl[this]"] /
                                       res["kernel_ms"]["plain[this]"], 4)
        for name in args.ref_lib:
            for kind in ("plain", "excl"):
                res[f"{kind}_over_{name}"] = round(res["kernel_ms"][f"{kind}[this]"] /
                                                   res["kernel_ms"][f"{kind}[{name}]"], 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
