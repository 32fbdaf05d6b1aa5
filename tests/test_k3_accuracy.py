"""K3's fp32-accuracy contract on the device (csrc/linear_common.h: the bf16x6 split keeps six
piece products in two fp32 accumulators and is as accurate as fp32), held three ways:

* every output element within ``BOUND`` = 8 units of ``u = 2^-24 (sum |x||w| + |bias|)`` of
  float64, per element and not per tensor maximum — a split that lost any one small piece
  product is at 9.5 u or more on the same inputs (test_k3_accuracy_ref.py, on the CPU);
* inputs built from signed powers of two and the constants c2 = 1 + 2^-9 (bf16 pieces
  1, 2^-9, 0) and c3 = c2 + 2^-18 (pieces 1, 2^-9, 2^-18) whose result is one known fp32 number:
  compared bitwise;
* rows scaled by 2^-60 .. 2^60: bitwise the scaled rows of the unscaled run.

Each on the split and on the f32-input kernels it replaces, through the single calls and the
two-job calls, forward, dgrad and wgrad.  The f32-input kernels are fp32 FMA chains: they round
where the split does not (a sum of more than 63 products (1 + 2^-9)^2 needs more than 24
bits), so with the split off the bitwise constructs are the ones whose partial sums are fp32
numbers in any order (c1 = 1 + 2^-7 in every column, c2 in one 16-column chunk), and c2 / c3 in
every column are held to a chain's a-priori bound in units instead (``_chain_bound``).
"""
import pytest
import torch

from oracle import split_ref as S

import k3_accuracy_cases as C
from k3_accuracy_cases import BOUND, H, MULTI

pytestmark = pytest.mark.gpu
DEV = "cuda"

PATH_SHAPES = [(True, ks, H) for ks in C.SPLIT_LAYOUTS] + [(False, ks, h) for ks, h in C.F32_SHAPES]
PATH_LAYOUTS = [(s, ks) for s in (True, False) for ks in C.SPLIT_LAYOUTS] + [(False, [64])]


def _id(v):
    if isinstance(v, bool):
        return "split" if v else "f32"
    if isinstance(v, (list, tuple)):
        return "+".join(str(k) for k in v)
    return str(v)


@pytest.fixture(scope="module")
def ops():
    from truth_recommendation_gnn_amd import ops as _ops
    return _ops


def _assert_units(units, what):
    print(what, {k: round(v, 3) for k, v in units.items()})
    for k, v in units.items():
        assert v <= BOUND, f"{what}: {k} is {v:.2f} u from float64, the bound is {BOUND} u"


# ---------------------------------------------------------------------------- §3: units
@pytest.mark.parametrize("n", C.ROWS + [MULTI], ids=_id)
@pytest.mark.parametrize("split,ks,h", PATH_SHAPES, ids=_id)
def test_every_element_within_the_bound_in_units(ops, split, ks, h, n):
    """Forward (bias, no activation), every dX segment, dW and db of seeded randn inputs
    (W = 0.2 randn): each element within BOUND units of float64, the unit being that element's
    own sum of |products|.  One row is drawn 16 times (C.DRAWS)."""
    with C.k3_split(split):
        for rep in range(C.draws(n)):
            _assert_units(C.case_units(C.run_case(ops, DEV, ks, h, n, rep)), f"{_id(ks)} n={n} #{rep}")


@pytest.mark.parametrize("split,ks,h", PATH_SHAPES, ids=_id)
def test_forward_with_added_rows_and_relu_bits_within_the_bound(ops, split, ks, h):
    """The forward with ``add=`` (its |add| enters the unit) and, where the output width has a
    bit form, ReLU and ``mask_out=``: within BOUND units of relu(float64), the bits equal to
    out > 0."""
    with C.k3_split(split):
        res = C.run_case(ops, DEV, ks, h, MULTI, add=True)
    _assert_units(C.case_units(res), f"{_id(ks)} add")
    assert res["relu"] == (h % 16 == 0 and h <= 128)
    if res["relu"]:
        assert torch.equal(res["mask"], res["out"] > 0)


@pytest.mark.parametrize("ks,ns", C.PAIRS, ids=_id)
@pytest.mark.parametrize("split", [True, False], ids=_id)
def test_two_job_calls_within_the_bound(ops, split, ks, ns):
    """linear_fwd_many / linear_bwd_many with two jobs of one K and different row counts
    (K = 512 on the split: k_lin_fwd_xs2 / k_lin_bwd_xs2 / k_wgrad_reduce2): each job held like
    a single call."""
    with C.k3_split(split):
        for j, res in enumerate(C.run_pair(ops, DEV, ks, ns)):
            _assert_units(C.case_units(res), f"{_id(ks)} job {j} n={ns[j]}")


# ---------------------------------------------------------------------------- §4: exact values
def _bitwise(got, want64, what):
    assert C.representable(want64), what
    want = want64.float()
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                             f"{i}: got {float(got[i])!r}, exact value {float(want[i])!r}")


def _fwd_variants(k):
    """(constant, constant columns): every column, and one 16-column chunk at each position."""
    v = [(c, None) for c in ("c1", "c2", "c3")]
    for c in ("c2", "c3"):
        v += [(c, list(range(16 * p, 16 * p + 16))) for p in C.chunk_positions(k)]
    return v


def _chain_bound(split, length):
    """The bound for a constant-input construct that is not a bitwise one on its path.  On the
    split that is BOUND (c1: one piece, nothing rounds).  An fp32 FMA chain rounds c2 / c3 in
    every column the same way at every step — the errors add up instead of averaging out, which
    the bound of 8 u for random inputs assumes — so there only the a-priori bound of ``length``
    additions of at most 2^-24 sum |x w| each holds: ``length`` units.  (A sequential fp32 FMA
    chain on the CPU is 31.9 u off at K = 128 and 55.8 u at K = 512 on these inputs, torch's
    fp32 mm 31.9 / 47.8 u; the f32-input kernels measured 31.9 / 55.8 u on the MI355X.)"""
    return BOUND if split else float(max(BOUND, length))


def _exact_on(split, e, key="span"):
    """Is the construct a bitwise one on this path?  On the split: c2 and c3 (hi and lo hold
    exact sums, hi + lo is the stated value).  On an fp32 FMA chain: when every partial sum in
    any order is an fp32 number."""
    return e["const"] in ("c2", "c3") if split else e[key] < 2.0 ** 24


@pytest.mark.parametrize("n", [1, 37, MULTI], ids=_id)
@pytest.mark.parametrize("split,ks", PATH_LAYOUTS, ids=_id)
def test_forward_exact_values(ops, split, ks, n):
    """x[r, k] = s_r p_k q_k, w[h, k] = t_h q_k / p_k (C.exact_product): the output is
    s_r t_h (n_c kept(c) + the other columns' 2^-12 each) + bias, bitwise, without and with ReLU
    (then +0 wherever that is not positive, and the bits equal to out > 0)."""
    k = sum(ks)
    with C.k3_split(split):
        for const, cols in _fwd_variants(k):
            e = C.exact_product(n, k, H, C.CONSTS[const], cols, bias=cols is None)
            e["const"] = const
            what = f"{_id(ks)} n={n} {const} cols={'all' if cols is None else cols[0]}"
            sd = C.segs_of(e["a"], ks, DEV)
            w, b = e["b"].to(DEV), e["bias"].to(DEV)
            out = ops.linear_fwd(sd, w, b, False).cpu()
            if not _exact_on(split, e):
                u = float(S.err_units(out, e["a"], e["b"], e["bias"]).max())
                assert u <= _chain_bound(split, k), f"{what}: {u:.2f} u"
                continue
            want = e["split"] if split else e["plain"]
            _bitwise(out, want, what)
            mk = ops.relu_mask_for(n, H, True, torch.device(DEV))
            act = ops.linear_fwd(sd, w, b, True, mask_out=mk).cpu()
            _bitwise(act, want.clamp_min(0.0), what + " relu")
            assert not bool(torch.signbit(act).any()), what + ": -0 after the ReLU"
            assert torch.equal(C.unpack_relu_bits(mk, n, H), act > 0), what + " bits"
            assert bool((want > 0).any()) and bool((want < 0).any())


@pytest.mark.parametrize("n", [1, 37, MULTI], ids=_id)
@pytest.mark.parametrize("split,ks", PATH_LAYOUTS, ids=_id)
def test_backward_exact_values(ops, split, ks, n):
    """dgrad: dz[r, h] = s_r p_h q_h, W[h, k] = t_k q_h / p_h, reduction over the 128 h.
    wgrad: dz[r, h] = a_r m_r u_h c, x[r, k] = a_r v_k q_k (C.exact_wgrad), reduction over the
    rows, with db = sum_r dz.  Bitwise where the path keeps every partial sum exact, else within
    the bound in units."""
    k = sum(ks)
    zeros = [torch.zeros(n, kk, device=DEV) for kk in ks]
    with C.k3_split(split):
        for const, cols in [(c, None) for c in ("c1", "c2", "c3")] + \
                [(c, list(range(16 * p, 16 * p + 16))) for c in ("c2", "c3") for p in (0, 7)]:
            e = C.exact_product(n, H, k, C.CONSTS[const], cols, bias=False)
            e["const"] = const
            what = f"dgrad {_id(ks)} n={n} {const} cols={'all' if cols is None else cols[0]}"
            w = e["b"].T.contiguous()
            dxs = [torch.full_like(z, 7.0) for z in zeros]
            ops.linear_bwd(zeros, w.to(DEV), e["a"].to(DEV), None, dxs, False, False)
            dx = torch.cat([t.cpu() for t in dxs], 1)
            if _exact_on(split, e):
                _bitwise(dx, e["split"] if split else e["plain"], what)
            else:
                u = float(S.err_units(dx, e["a"], e["b"]).max())
                assert u <= _chain_bound(split, H), f"{what}: {u:.2f} u"
        wz = torch.zeros(H, k, device=DEV)
        for const, cols in [(c, None) for c in ("c1", "c2", "c3")] + \
                [(c, list(range(16 * p, 16 * p + 16))) for c in ("c2", "c3")
                 for p in C.chunk_positions(k)]:
            e = C.exact_wgrad(n, k, H, C.CONSTS[const], cols)
            e["const"] = const
            what = f"wgrad {_id(ks)} n={n} {const} cols={'all' if cols is None else cols[0]}"
            # the condition for the row weights, from the integers: at most 63 rows of weight 1,
            # or 32-row tiles of 64 each, at most 63 of them
            m = [int(v) for v in e["m"]]
            tiles = [sum(m[r:r + 32]) for r in range(0, n, 32)]
            assert (n <= 63 and set(m) == {1}) or (set(tiles) == {64} and len(tiles) <= 63)
            total = sum(m) * (2 ** 18 + 2 ** 10 + 3)
            assert (total // (total & -total)).bit_length() <= 24
            dw, db = ops.linear_bwd(C.segs_of(e["x"], ks, DEV), wz, e["dz"].to(DEV), None,
                                    [None] * len(ks), True, True)
            dw, db = dw.cpu(), db.cpu()
            if _exact_on(split, e, "dw_span"):
                _bitwise(dw, e["dw_split"] if split else e["dw_plain"], what)
            else:
                u = float(S.err_units(dw, e["dz"].T.contiguous(), e["x"].T.contiguous()).max())
                assert u <= _chain_bound(split, n), f"{what}: {u:.2f} u"
            if e["db_span"] < 2.0 ** 24:      # plain fp32 sums on every path
                _bitwise(db, e["db"], what + " db")
            else:
                u = float(S.err_units(db.reshape(1, -1), torch.ones(1, n),
                                      e["dz"].T.contiguous()).max())
                assert u <= _chain_bound(False, n), f"{what} db: {u:.2f} u"


@pytest.mark.parametrize("ks,ns", C.PAIRS, ids=_id)
def test_two_job_calls_exact_values(ops, ks, ns):
    """The exact constructs (c2 and c3 in every column) through linear_fwd_many /
    linear_bwd_many on the split: both jobs' outputs, dX and dW bitwise."""
    k = sum(ks)
    for const in ("c2", "c3"):
        c = C.CONSTS[const]
        fw = [C.exact_product(n, k, H, c, None, row_mix=bool(j)) for j, n in enumerate(ns)]
        jobs = [(C.segs_of(e["a"], ks, DEV), e["b"].to(DEV), e["bias"].to(DEV), False, None)
                for e in fw]
        with C.k3_split(True):
            outs = ops.linear_fwd_many(jobs)
        for j, (e, o) in enumerate(zip(fw, outs)):
            _bitwise(o.cpu(), e["split"], f"pair {_id(ks)} {const} job {j} out")
        dg = [C.exact_product(n, H, k, c, None, bias=False) for n in ns]
        wg = [C.exact_wgrad(n, k, H, c) for n in ns]
        # one backward per job pair for the dgrad (its own W) and one for the wgrad (its own x)
        bj = [([torch.zeros(n, kk, device=DEV) for kk in ks], e["b"].T.contiguous().to(DEV),
               e["a"].to(DEV), None, [torch.empty(n, kk, device=DEV) for kk in ks], False, False,
               None) for e, n in zip(dg, ns)]
        bw = [(C.segs_of(e["x"], ks, DEV), torch.zeros(H, k, device=DEV), e["dz"].to(DEV), None,
               [None] * len(ks), True, True, None) for e in wg]
        with C.k3_split(True):
            ops.linear_bwd_many(bj)
            grads = ops.linear_bwd_many(bw)
        for j, (e, job) in enumerate(zip(dg, bj)):
            _bitwise(torch.cat([t.cpu() for t in job[4]], 1), e["split"],
                     f"pair {_id(ks)} {const} job {j} dX")
        for j, (e, (dw, db)) in enumerate(zip(wg, grads)):
            _bitwise(dw.cpu(), e["dw_split"], f"pair {_id(ks)} {const} job {j} dW")


# ---------------------------------------------------------------------------- §5: mixed rows
MIXED = [(s, ks, H) for s in (True, False) for ks in ([128], [128, 128], [128, 128, 128, 128])] + \
    [(False, [3, 5], 7)]


@pytest.mark.parametrize("split,ks,h", MIXED, ids=_id)
def test_rows_of_mixed_magnitude(ops, split, ks, h):
    """Row r of X (forward) and of dout (backward) times 2^e_r, e_r cycling through
    -60, -20, 0, 20, 60 inside every row tile: output row r and dX row r are bitwise 2^e_r
    times the unscaled run's (no bias: a power of two commutes with every rounding as long as
    nothing leaves the normal range, asserted on the float64 reference), and each row meets the
    bound in its own units.  dW / db: rows scaled by 2^-8, 1, 2^8, in units."""
    n = MULTI
    d = C.draw(ks, h, n, rep=200)
    sc = C.row_scales(n, C.ROW_EXPS)
    # the precondition: the smallest product piece the split forms (third order: 2^-18 of
    # |x||w| at most 2 bits below) stays normal, the largest output stays finite
    xd, wd, zd = d["x"].double(), d["w"].double(), d["dout"].double()
    tiny = 2.0 ** min(C.ROW_EXPS) * 2.0 ** -20
    assert float(xd.abs().min()) * float(wd.abs().min()) * tiny >= 2.0 ** -126
    assert float(zd.abs().min()) * float(wd.abs().min()) * tiny >= 2.0 ** -126
    big = 2.0 ** max(C.ROW_EXPS)
    assert float((xd.abs() @ wd.abs().T).max()) * big < 2.0 ** 127
    assert float((zd.abs() @ wd.abs()).max()) * big < 2.0 ** 127
    xs, zs = (xd * sc[:, None]).float(), (zd * sc[:, None]).float()
    assert torch.equal(xs.double(), xd * sc[:, None]) and torch.equal(zs.double(), zd * sc[:, None])
    w = d["w"].to(DEV)

    def run(x, dout):
        sd = C.segs_of(x, ks, DEV)
        out = ops.linear_fwd(sd, w, None, False).cpu()
        dxs = [torch.empty_like(s) for s in sd]
        dw, db = ops.linear_bwd(sd, w, dout.to(DEV), None, dxs, True, True)
        return out, torch.cat([t.cpu() for t in dxs], 1), dw.cpu(), db.cpu()

    with C.k3_split(split):
        out0, dx0, _, _ = run(d["x"], d["dout"])
        out1, dx1, _, _ = run(xs, zs)
        # dW / db: x rows by 2^e_r, dout rows by 2^e_(r+1), e in -8, 0, 8
        s8 = C.row_scales(n + 1, C.WGRAD_EXPS)
        x8, z8 = (xd * s8[:n, None]).float(), (zd * s8[1:, None]).float()
        _, _, dw8, db8 = run(x8, z8)
    f32 = lambda t: t.float()  # noqa: E731
    assert torch.equal(out1, f32(out0.double() * sc[:, None]))
    assert torch.equal(dx1, f32(dx0.double() * sc[:, None]))
    units = {"out": float(S.err_units(out1, xs, d["w"]).max()),
             "dx": float(S.err_units(dx1, zs, d["w"].T.contiguous()).max())}
    units.update({k: float(v.max()) for k, v in
                  C.bwd_units(None, dw8, db8, {"x": x8, "dout": z8, "w": d["w"]}).items()})
    _assert_units(units, f"{_id(ks)} mixed rows")
