"""The bf16x6 split of K3 in plain torch on the CPU — TEST INFRASTRUCTURE ONLY.

``csrc/linear_common.h`` states the contract of the split kernels: every fp32 value is three bf16
pieces, a product is the six piece products whose orders add to at most 4, the large product
(``x1w1``) and the five small ones accumulate in two fp32 accumulators, and the result is
``hi + lo``.  This module writes that arithmetic down independently of the kernels (pieces via
``.bfloat16()``, products and 32-column sums in float64, one fp32 rounding per accumulate) and
measures any result, a kernel's or the emulation's, in units of
``u = 2^-24 (sum_k |x_k| |w_k| + |bias|)`` per output element against float64.

Used by ``tests/test_k3_accuracy*.py`` and ``scripts/k3_accuracy.py``; never by the package.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

# the six piece products, in the order x6_mma issues them: lo takes the first five, hi the last
SIX = ("x2w2", "x1w3", "x3w1", "x1w2", "x2w1", "x1w1")
SMALL = SIX[:5]


def pieces(v: torch.Tensor):
    """The three bf16 pieces of fp32 ``v`` as float64: v1 = bf16(v), v2 = bf16(v - v1),
    v3 = bf16(v - v1 - v2), each rounded to nearest even (the residuals are exact in fp32)."""
    v = v.detach().to(torch.float32).cpu()
    v1 = v.bfloat16().float()
    r1 = v - v1
    v2 = r1.bfloat16().float()
    r2 = r1 - v2
    v3 = r2.bfloat16().float()
    return v1.double(), v2.double(), v3.double()


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()          # one rounding to fp32, kept as float64


def split_matmul(x: torch.Tensor, w: torch.Tensor, terms: Sequence[str] = SIX, step: int = 32,
                 flush: Optional[int] = None) -> torch.Tensor:
    """``x @ w.T`` ([n, K] by [H, K]) as the split computes it, returned as fp32.

    ``hi`` accumulates ``x1w1`` and ``lo`` the small products, each an fp32 accumulator that takes
    one ``step``-column partial product (exact, as float64) per piece product at a time, in the
    order of ``SIX``; the result is ``hi + lo`` rounded once.  ``terms`` names the products kept:
    leaving one out is the defect the accuracy tests must catch.  ``flush``: after every
    ``flush`` columns ``hi + lo`` is rounded and added into a running fp32 total and both
    accumulators restart — the kernels' order where one accumulator pair does not span the whole
    reduction (the forward's column blocks of 256 at K = 384 / 512; the wgrad's 32-row tiles)."""
    for t in terms:
        if t not in SIX:
            raise ValueError(f"unknown piece product {t!r}")
    xp, wp = pieces(x), pieces(w)
    n, k = x.shape
    h = w.shape[0]
    zero = lambda: torch.zeros(n, h, dtype=torch.float64)  # noqa: E731
    hi, lo, total = zero(), zero(), None
    for c0 in range(0, k, step):
        c1 = min(c0 + step, k)
        for t in SIX:
            if t not in terms:
                continue
            p = xp[int(t[1]) - 1][:, c0:c1] @ wp[int(t[3]) - 1][:, c0:c1].T
            if t == "x1w1":
                hi = _f32(hi + p)
            else:
                lo = _f32(lo + p)
        if flush is not None and (c1 % flush == 0 or c1 == k):
            part = _f32(hi + lo)
            total = part if total is None else _f32(total + part)
            hi, lo = zero(), zero()
    if flush is None:
        total = _f32(hi + lo)
    return total.float()


def _addends(bias):
    if bias is None:
        return []
    return [t.detach().cpu().double() for t in (bias if isinstance(bias, (list, tuple)) else [bias])]


def unit(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """``u = 2^-24 (sum_k |x_k| |w_k| + |bias|)`` per element of ``x @ w.T`` (+ ``bias``: a row
    of H values, a whole [n, H] addend, or a list of such, each entering as its own ``|.|``),
    in float64."""
    s = x.detach().cpu().double().abs() @ w.detach().cpu().double().abs().T
    for t in _addends(bias):
        s = s + t.abs()
    return s * 2.0 ** -24


def err_units(got: torch.Tensor, x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """Per element, ``|got - ref64| / u`` with ``ref64 = x @ w.T (+ bias)`` in float64 and ``u``
    from :func:`unit`; an element whose unit is 0 (every product 0) must be exactly ``ref64``
    and counts as 0 then, as inf otherwise."""
    xd, wd = x.detach().cpu().double(), w.detach().cpu().double()
    ref = xd @ wd.T
    for t in _addends(bias):
        ref = ref + t
    u = unit(x, w, bias)
    d = (got.detach().cpu().double() - ref).abs()
    e = d / u.clamp_min(torch.finfo(torch.float64).tiny)
    return torch.where(u > 0, e, torch.where(d == 0, torch.zeros_like(d),
                                             torch.full_like(d, float("inf"))))
