"""Inputs, cases and reference arithmetic shared by ``test_k3_accuracy.py`` (GPU),
``test_k3_accuracy_ref.py`` (CPU: the same inputs through ``oracle/split_ref.py``, to show the
GPU checks separate a correct split from one that lost a piece product) and
``scripts/k3_accuracy.py`` (the measured maxima of ``profiles/k3_accuracy.jsonl``).

Everything here is plain torch on the CPU; the functions that run K3 take ``ops`` and the
device as arguments.
"""
from __future__ import annotations

import contextlib
import math

import torch

from oracle import split_ref as S

# ---------------------------------------------------------------------------- §3: error in units
# The bound on |got - float64| in units of u = 2^-24 (sum |x||w| + |bias| + |add|), per element.
# Not taken from the kernels: fp32 torch.mm on the CPU peaks at 5.4 u on these inputs, the
# emulated correct split at 1.6 u, and the emulated split with any one of the five small piece
# products removed at 9.5 u or more at every case below (test_k3_accuracy_ref.py).
BOUND = 8.0

H = 128
SPLIT_LAYOUTS = [[128], [128, 128], [64, 64, 128], [128, 128, 128], [64, 256, 64],
                 [128, 128, 128, 128]]
# split off: the same layouts on the f32-input kernels (v4 / v5 up to K = 256, the general ones
# above), plus the v4 / v5 families at other shapes and the general kernels
F32_SHAPES = [(ks, H) for ks in SPLIT_LAYOUTS] + [([64, 64], 64), ([64], 128), ([3, 5], 7),
                                                  ([16], 200)]
ROWS = [1, 37, 512]
MULTI = 64 * 5 + 29          # several row tiles (32 and 64 rows) with a ragged tail
# A single row has 128 outputs, too few for the largest of them to show a lost third-order
# product at K = 384 / 512 (5.7 u); 16 independent draws of the one-row problem do (9.5 u).
DRAWS = {1: 16}
# two jobs of one K through linear_fwd_many / linear_bwd_many: K = 512 shares each column
# block's launch (k_lin_*_xs2), K = 256 runs job by job
PAIRS = [([128, 128], (37, MULTI)), ([128, 128, 128, 128], (MULTI, 37))]


def draws(n):
    return DRAWS.get(n, 1)


def draw(ks, h, n, rep=0):
    """Seeded unit-scale inputs of one K3 problem: the concatenated X [n, K], W = 0.2 randn
    [h, K], bias, the added rows and dout.  The seed depends on (K, h, n, rep) only, so every
    segment layout of one K sees the same numbers."""
    k = sum(ks)
    g = torch.Generator().manual_seed(((k * 1009 + h) * 4099 + n) * 17 + rep)
    return {"x": torch.randn(n, k, generator=g), "w": torch.randn(h, k, generator=g) * 0.2,
            "b": torch.randn(h, generator=g), "add": torch.randn(n, h, generator=g),
            "dout": torch.randn(n, h, generator=g)}


@contextlib.contextmanager
def k3_split(on):
    """K3 at H = 128 on the bf16x6 split (True, the default) or on the f32-input kernels; the
    previous setting is restored (the pattern of ``_k3_split`` in test_gpu_parity.py)."""
    from truth_recommendation_gnn_amd import _native as N
    prev = N.lib().hgnn_set_k3_split(int(on))
    try:
        yield
    finally:
        N.lib().hgnn_set_k3_split(prev)


def segs_of(x, ks, dev):
    return [s.contiguous().to(dev) for s in x.split(ks, 1)]


def unpack_relu_bits(mask, n, h):
    """hgnn_linear_fwd_mask's lane layout as a dense [n, h] bool: word row * 4 + g, bit 4 c + e
    is column 16 c + 4 g + e."""
    m = mask.cpu().view(torch.int32).reshape(n, 4).to(torch.int64) & 0xFFFFFFFF
    out = torch.zeros(n, h, dtype=torch.bool)
    for g in range(4):
        for c in range(h // 16):
            for e in range(4):
                out[:, 16 * c + 4 * g + e] = ((m[:, g] >> (4 * c + e)) & 1).bool()
    return out


def fwd_units(out, d, add=None, relu=False):
    """Forward error per element in units of 2^-24 (sum |x||w| + |b| (+ |add|)).  With a ReLU
    the reference is relu(float64): ReLU moves no two numbers further apart."""
    terms = [d["b"]] if add is None else [d["b"], add]
    if not relu:
        return S.err_units(out, d["x"], d["w"], terms)
    ref = d["x"].double() @ d["w"].double().T + sum(t.double() for t in terms)
    return (out.cpu().double() - ref.clamp_min(0)).abs() / S.unit(d["x"], d["w"], terms)


def bwd_units(dx, dw, db, d):
    """Backward errors (no activation mask: dz = dout) in their own units: dX against
    dz W (units from |dz||W|), dW against dz^T X (sum_r |dz||x|), db against sum_r dz
    (sum_r |dz|)."""
    res = {}
    if dx is not None:
        res["dx"] = S.err_units(dx, d["dout"], d["w"].T.contiguous())
    if dw is not None:
        res["dw"] = S.err_units(dw, d["dout"].T.contiguous(), d["x"].T.contiguous())
    if db is not None:
        ones = torch.ones(1, d["dout"].shape[0])
        res["db"] = S.err_units(db.reshape(1, -1), ones, d["dout"].T.contiguous())
    return res


def run_case(ops, dev, ks, h, n, rep=0, add=False, d=None):
    """One K3 forward and backward on the device (the K3 path is the caller's ``k3_split``),
    no activation; with ``add`` the forward takes the added rows and, where the shape has a
    bit form, a ReLU with ``mask_out``.  Returns the outputs on the CPU."""
    d = d or draw(ks, h, n, rep)
    sd = segs_of(d["x"], ks, dev)
    w, b = d["w"].to(dev), d["b"].to(dev)
    res = {"d": d}
    if add:
        mk = ops.relu_mask_for(n, h, True, torch.device(dev))
        relu = mk is not None
        out = ops.linear_fwd(sd, w, b, relu, add=d["add"].to(dev), mask_out=mk)
        res.update(out=out.cpu(), relu=relu, mask=None if mk is None else unpack_relu_bits(mk, n, h))
        return res
    res["out"] = ops.linear_fwd(sd, w, b, False).cpu()
    dxs = [torch.empty_like(s) for s in sd]
    dw, db = ops.linear_bwd(sd, w, d["dout"].to(dev), None, dxs, True, True)
    res.update(dx=torch.cat([t.cpu() for t in dxs], 1), dw=dw.cpu(), db=db.cpu())
    return res


def case_units(res):
    """Max error in units per output of a :func:`run_case` result."""
    d = res["d"]
    if "dx" not in res:
        return {"out_add": float(fwd_units(res["out"], d, d["add"], res["relu"]).max())}
    m = {"out": float(fwd_units(res["out"], d).max())}
    m.update({k: float(v.max()) for k, v in bwd_units(res["dx"], res["dw"], res["db"], d).items()})
    return m


def run_pair(ops, dev, ks, ns):
    """Two jobs of one K through linear_fwd_many / linear_bwd_many; a :func:`run_case`-shaped
    result per job."""
    ds = [draw(ks, H, n, rep=100 + j) for j, n in enumerate(ns)]
    jobs = [(segs_of(d["x"], ks, dev), d["w"].to(dev), d["b"].to(dev), False, None) for d in ds]
    outs = ops.linear_fwd_many(jobs)
    bj = [(j[0], j[1], d["dout"].to(dev), None, [torch.empty_like(s) for s in j[0]], True, True,
           None) for j, d in zip(jobs, ds)]
    grads = ops.linear_bwd_many(bj)
    return [{"d": d, "out": o.cpu(), "dx": torch.cat([t.cpu() for t in j[4]], 1),
             "dw": dw.cpu(), "db": db.cpu()} for d, o, j, (dw, db) in zip(ds, outs, bj, grads)]


# ---------------------------------------------------------------------------- §4: exact values
# c2 = 1 + 2^-9 has the bf16 pieces (1, 2^-9, 0), c3 = 1 + 2^-9 + 2^-18 the pieces
# (1, 2^-9, 2^-18).  c1 = 1 + 2^-7 is one bf16 piece: its square has 15 bits, so a sum of up to
# 512 of them is an fp32 number in any order (the f32-input kernels' exact construct).
C1 = 1.0 + 2.0 ** -7
C2 = 1.0 + 2.0 ** -9
C3 = 1.0 + 2.0 ** -9 + 2.0 ** -18
CONSTS = {"c1": C1, "c2": C2, "c3": C3}


def kept(c):
    """The part of c * c the split keeps: the piece products whose orders add to at most 4."""
    p = [float(t) for t in S.pieces(torch.tensor([c]))]
    return sum(p[i] * p[j] for i in range(3) for j in range(3) if i + j <= 2)


def pow2_cycle(n, exps, sign_period=None):
    """n signed powers of two: exponents cycling through ``exps``, the sign flipping with
    ``sign_period`` (None: all positive)."""
    v = torch.tensor([2.0 ** exps[i % len(exps)] for i in range(n)], dtype=torch.float64)
    if sign_period:
        v = v * torch.tensor([-1.0 if (i // sign_period) % 2 else 1.0 for i in range(n)],
                             dtype=torch.float64)
    return v


def chunk_positions(k):
    """The 16-column chunks a routing variant puts the constant in: the first, the last, and
    the two on either side of column 256 (the column blocks' edge) where K reaches it."""
    pos = [0, k // 16 - 1]
    if k > 256:
        pos += [15, 16]
    return pos


def exact_product(n, k, h, c, cols=None, bias=True, row_mix=True):
    """An exact-value problem ``A [n, k]``, ``B [h, k]`` (and a bias) for ``A @ B.T + bias``:
    ``A[r, j] = s_r p_j q_j`` and ``B[i, j] = t_i q_j / p_j`` with s, t, p signed powers of two,
    so every product is ``s_r t_i q_j^2``; ``q_j = c`` on the columns ``cols`` (all by default)
    and ``2^-6`` on the others, which then add ``2^-12`` each.  The per-column scale p (undone
    in B) makes a column paired with the wrong weight column show.  Returns fp32 tensors and
    the float64 value the split must give exactly (``kept(c)`` per constant column) and the
    one plain fp32 / float64 arithmetic gives (``c * c``)."""
    s = pow2_cycle(n, [0, 1, -2, 2, -1], 3 if row_mix else None)
    t = pow2_cycle(h, [1, -1, 0, -2, 2, 0, 1], 5)
    p = pow2_cycle(k, [0, 2, -1, 1, -2])
    q = torch.full((k,), c if cols is None else 2.0 ** -6, dtype=torch.float64)
    if cols is not None:
        q[cols] = c
    a = (s[:, None] * (p * q)[None, :]).float()
    b = (t[:, None] * (q / p)[None, :]).float()
    assert torch.equal(a.double(), s[:, None] * (p * q)[None, :])      # fp32 holds them exactly
    assert torch.equal(b.double(), t[:, None] * (q / p)[None, :])
    n_c = k if cols is None else len(cols)
    other = (k - n_c) * 2.0 ** -12
    bv = torch.tensor([[0.0, 1.0, -2.0, 2.0 ** -5][i % 4] if bias else 0.0 for i in range(h)],
                      dtype=torch.float64)
    st = s[:, None] * t[None, :]
    return {"a": a, "b": b, "bias": bv.float(),
            "split": st * (n_c * kept(c) + other) + bv,
            "plain": st * (n_c * c * c + other) + bv,
            # sum of |products| (+ |bias|) over the lowest bit any of them has: below 2^24,
            # every partial sum in any order is an fp32 number
            "span": _span(st, n_c, c, k - n_c, bv)}


def _low_bit(v: float) -> float:
    """The lowest set bit of a double (inf for 0)."""
    if v == 0.0:
        return math.inf
    m, e = math.frexp(abs(v))
    mi = int(m * 2 ** 53)
    return math.ldexp(mi & -mi, e - 53)


def _span(st, n_c, c, n_other, bv):
    lb = min(_low_bit(c * c) if n_c else math.inf, 2.0 ** -12 if n_other else math.inf)
    tot = n_c * c * c + n_other * 2.0 ** -12
    low = torch.minimum(st.abs() * lb, torch.tensor([_low_bit(float(v)) for v in bv])[None, :])
    return float(((st.abs() * tot + bv.abs()[None, :]) / low).max())


def wgrad_row_weights(n):
    """Row weights (powers of two) for the exact wgrad: 1 for n <= 63 rows; for more rows every
    32-row tile, the ragged last one included, sums to 64, so any union of whole tiles is
    64 m with m <= 63 and m (2^18 + 2^10 + 3) has at most 24 significant bits."""
    if n <= 63:
        return [1] * n
    wts = []
    for r0 in range(0, n, 32):
        rows = min(32, n - r0)
        tile = [64]                      # split the largest weight until there is one per row
        while len(tile) < rows:
            tile.sort()
            big = tile.pop()
            tile += [big // 2, big // 2]
        wts += sorted(tile)
    return wts


def exact_wgrad(n, k, h, c, cols=None):
    """dz [n, h] and x [n, k] for the exact wgrad: ``dz[r, i] = a_r m_r u_i c`` and
    ``x[r, j] = a_r v_j q_j`` with a_r = -1 on every third row (a row of dz paired with another row of x
    changes sign), m_r the row weights, u, v signed powers of two, q_j = c on ``cols`` (all by default)
    and 1 elsewhere.  dW[i, j] = M u_i v_j c q_j with M = sum m_r; db[i] = sum_r a_r m_r u_i c."""
    m = torch.tensor(wgrad_row_weights(n), dtype=torch.float64)
    a = torch.tensor([-1.0 if r % 3 == 2 else 1.0 for r in range(n)], dtype=torch.float64)
    u = pow2_cycle(h, [1, -1, 0, -2, 2, 0, 1], 5)
    v = pow2_cycle(k, [0, 2, -1, 1, -2], 7)
    q = torch.full((k,), c if cols is None else 1.0, dtype=torch.float64)
    if cols is not None:
        q[cols] = c
    dz = ((a * m)[:, None] * u[None, :] * c).float()
    x = (a[:, None] * (v * q)[None, :]).float()
    p = [float(t) for t in S.pieces(torch.tensor([c]))]
    k_cc = kept(c)
    k_c1 = c                              # c times a power of two: the three pieces of c, all kept
    big = float(m.sum())
    uv = u[:, None] * v[None, :]
    is_c = (q == c)[None, :]
    return {"dz": dz, "x": x, "m": m, "pieces": p,
            "dw_split": big * uv * _where(is_c, k_cc, k_c1),
            "dw_plain": big * uv * _where(is_c, c * c, c),
            "db": (a * m).sum() * u * c + 0.0,
            # |partial sums| of dW over the lowest product bit, for any order of the rows
            "dw_span": big / float(m.min()) * c * c / _low_bit(c * c),
            "db_span": float(m.sum()) / float(m.min()) * c / _low_bit(c)}


def _where(cond, a: float, b: float):
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    return torch.where(cond, f64(a), f64(b))


def representable(v64):
    return bool(torch.equal(v64.float().double(), v64))


# ---------------------------------------------------------------------------- §5: mixed rows
ROW_EXPS = [-60, -20, 0, 20, 60]     # X / dout row r times 2^e, cycling inside every row tile
WGRAD_EXPS = [-8, 0, 8]              # dW / db: bounded, so a few rows do not own the unit


def row_scales(n, exps):
    return torch.tensor([2.0 ** exps[r % len(exps)] for r in range(n)], dtype=torch.float64)
