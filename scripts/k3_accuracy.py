#!/usr/bin/env python3
"""K3's measured error per path, shape and output, in units of 2^-24 (sum |x||w| + |bias|)
against float64: the inputs and helpers of tests/test_k3_accuracy.py, one GPU run, one JSON
line per (path, shape, n) with the maximum over that case's elements (and draws).

    python scripts/k3_accuracy.py > profiles/k3_accuracy.jsonl
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import k3_accuracy_cases as C  # noqa: E402
from truth_recommendation_gnn_amd import ops  # noqa: E402

DEV = "cuda"


def emit(path, form, ks, h, n, units):
    print(json.dumps({"path": "split" if path else "f32", "form": form, "ks": ks, "h": h, "n": n,
                      "bound_u": C.BOUND, "max_u": {k: round(v, 3) for k, v in units.items()}}),
          flush=True)


def main():
    for split in (True, False):
        shapes = [(ks, C.H) for ks in C.SPLIT_LAYOUTS] if split else C.F32_SHAPES
        with C.k3_split(split):
            for ks, h in shapes:
                for n in C.ROWS + [C.MULTI]:
                    worst = {}
                    for rep in range(C.draws(n)):
                        for k, v in C.case_units(C.run_case(ops, DEV, ks, h, n, rep)).items():
                            worst[k] = max(worst.get(k, 0.0), v)
                    emit(split, "single", ks, h, n, worst)
                emit(split, "single+add", ks, h, C.MULTI,
                     C.case_units(C.run_case(ops, DEV, ks, h, C.MULTI, add=True)))
            for ks, ns in C.PAIRS:
                for n, res in zip(ns, C.run_pair(ops, DEV, ks, ns)):
                    emit(split, "two-job", ks, C.H, n, C.case_units(res))


if __name__ == "__main__":
    main()
