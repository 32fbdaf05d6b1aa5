"""CPU half of the K3 accuracy tests: the inputs test_k3_accuracy.py gives the device, through
the plain-torch emulation of the bf16x6 split (oracle/split_ref.py).  No project kernel runs
here.  It shows, without a GPU, that the device checks have teeth:

* with all six piece products the emulation stays within the bound at every shape, row count
  and orientation (forward, dgrad over H = 128, wgrad over the rows) the device tests use, and
  with any single one of the five small products removed it exceeds the bound at each of them;
* every exact-value construct is what it claims: exactly representable, equal to the emulation
  and to float64 rounded once to fp32, and — where the f32-input kernels are held bitwise —
  with every partial sum an fp32 number in any order.
"""
import pytest
import torch

from oracle import split_ref as S

import k3_accuracy_cases as C
from k3_accuracy_cases import BOUND, H, MULTI

KS = [128, 256, 384, 512]


def _f32(t):
    return t.float()


def _emulate(d, terms, add=False):
    """The split's outputs for one drawn problem, in the kernels' accumulation order: the
    forward in column blocks of 256, the wgrad in 32-row tiles."""
    k = d["x"].shape[1]
    z = _f32(S.split_matmul(d["x"], d["w"], terms, flush=256 if k > 256 else None).double()
             + d["b"].double())
    if add:
        return {"out": _f32(z.double() + d["add"].double()).clamp_min(0), "relu": True, "d": d}
    return {"out": z, "d": d,
            "dx": S.split_matmul(d["dout"], d["w"].T.contiguous(), terms),
            "dw": S.split_matmul(d["dout"].T.contiguous(), d["x"].T.contiguous(), terms, flush=32),
            "db": _f32(d["dout"].double().sum(0))}


def _teeth(problems, add=False):
    """Max units per output over the problems: all six products, and each small one removed."""
    def worst(terms):
        m = {}
        for d in problems:
            for key, v in C.case_units(_emulate(d, terms, add)).items():
                m[key] = max(m.get(key, 0.0), v)
        return m
    full = worst(S.SIX)
    for key, v in full.items():
        assert v <= BOUND, (key, v)
    split_outputs = [key for key in full if key != "db"]      # db is a plain sum: no pieces
    for t in S.SMALL:
        lost = worst([s for s in S.SIX if s != t])
        for key in split_outputs:
            assert lost[key] > BOUND, f"{key} without {t}: {lost[key]:.2f} u does not exceed {BOUND}"
    return full


@pytest.mark.parametrize("n", C.ROWS + [MULTI])
@pytest.mark.parametrize("k", KS)
def test_six_products_within_the_bound_and_any_five_beyond(k, n):
    _teeth([C.draw([k], H, n, rep) for rep in range(C.draws(n))])


@pytest.mark.parametrize("k", KS)
def test_added_rows_and_relu_keep_the_separation(k):
    _teeth([C.draw([k], H, MULTI)], add=True)


@pytest.mark.parametrize("ks,ns", C.PAIRS)
def test_two_job_inputs_keep_the_separation(ks, ns):
    for j, n in enumerate(ns):
        _teeth([C.draw(ks, H, n, rep=100 + j)])


def test_cases_cover_the_layouts_of_every_k():
    assert sorted({sum(ks) for ks in C.SPLIT_LAYOUTS}) == KS
    assert all(sum(ks) in KS for ks, _ in C.PAIRS)


def test_plain_fp32_reference_is_within_the_bound():
    """fp32 torch.mm on the CPU — the accuracy the split claims to match — meets the bound too:
    the bound does not ask more of the kernels than fp32 gives."""
    for k in KS:
        d = C.draw([k], H, 512)
        got = {"d": d, "out": d["x"] @ d["w"].T + d["b"], "dx": d["dout"] @ d["w"],
               "dw": d["dout"].T @ d["x"], "db": d["dout"].sum(0)}
        for key, v in C.case_units(got).items():
            assert v <= BOUND, (k, key, v)


# ---------------------------------------------------------------------------- the helper itself
def test_pieces_of_the_constants():
    for c, want in ((C.C1, (C.C1, 0.0, 0.0)), (C.C2, (1.0, 2.0 ** -9, 0.0)),
                    (C.C3, (1.0, 2.0 ** -9, 2.0 ** -18))):
        assert tuple(float(p) for p in S.pieces(torch.tensor([c]))) == want
    assert C.kept(C.C2) == C.C2 * C.C2 == 1 + 2.0 ** -8 + 2.0 ** -18
    assert C.kept(C.C3) == 1 + 2.0 ** -8 + 3 * 2.0 ** -18
    assert C.C3 * C.C3 - C.kept(C.C3) == 2.0 ** -26 + 2.0 ** -36


def test_pieces_rebuild_fp32_values():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 37.0
    p1, p2, p3 = S.pieces(v)
    for p in (p1, p2, p3):
        assert torch.equal(p.bfloat16().double(), p)
    assert float(((p1 + p2 + p3 - v.double()).abs() / v.double().abs()).max()) <= 2.0 ** -23


def test_err_units_counts_in_units_of_the_element():
    x = torch.tensor([[1.0, 2.0], [2.0 ** -40, 0.0]])
    w = torch.tensor([[3.0, -1.0]])
    ref = x.double() @ w.double().T
    assert float(S.err_units(ref.float(), x, w).max()) == 0.0
    off = (ref + torch.tensor([[5.0], [3.0 * 2.0 ** -40]]) * 2.0 ** -24 * 4.0).float()
    # row 0: 4 units of 2^-24 * 5; row 1: 4 units of 2^-24 * 3 * 2^-40, however small
    e = S.err_units(off, x, w)
    assert float(e[0, 0]) == 4.0 and float(e[1, 0]) == 4.0
    assert float(S.err_units(ref.float() + 1.0, x, w, torch.tensor([-1.0])).max()) > 1e6


def test_split_matmul_without_a_large_product_is_far_off():
    d = C.draw([128], H, 37)
    for t in ("x1w2", "x2w1"):
        got = S.split_matmul(d["x"], d["w"], [s for s in S.SIX if s != t])
        assert float(S.err_units(got, d["x"], d["w"]).max()) > 1000.0


# ---------------------------------------------------------------------------- exact constructs
def _chunk(p):
    return list(range(16 * p, 16 * p + 16))


@pytest.mark.parametrize("n", [1, 37, MULTI])
@pytest.mark.parametrize("k", KS)
def test_forward_constructs_give_the_stated_values(k, n):
    """c2 / c3 in every column or in one chunk: the value is an fp32 number, the emulation
    gives it bit for bit, and so does float64 rounded once.  In every column without a bias
    it is s t K (1 + 2^-8 + 2^-18) and s t K (1 + 2^-8 + 3 2^-18)."""
    variants = [(c, None) for c in ("c2", "c3")] + \
        [(c, _chunk(p)) for c in ("c2", "c3") for p in C.chunk_positions(k)]
    for const, cols in variants:
        e = C.exact_product(n, k, H, C.CONSTS[const], cols, bias=cols is None)
        assert C.representable(e["split"]) and float(e["split"].abs().min()) > 0
        want = e["split"].float()
        emu = _f32(S.split_matmul(e["a"], e["b"], flush=256 if k > 256 else None).double()
                   + e["bias"].double())
        assert torch.equal(emu, want), (const, cols)
        once = _f32(e["a"].double() @ e["b"].double().T + e["bias"].double())
        assert torch.equal(once, want), (const, cols)
        assert torch.equal(e["plain"], e["a"].double() @ e["b"].double().T + e["bias"].double())
    for const, extra in (("c2", 2.0 ** -18), ("c3", 3 * 2.0 ** -18)):
        e = C.exact_product(n, k, H, C.CONSTS[const], None, bias=False)
        st = C.pow2_cycle(n, [0, 1, -2, 2, -1], 3)[:, None] * \
            C.pow2_cycle(H, [1, -1, 0, -2, 2, 0, 1], 5)[None, :]
        assert torch.equal(e["split"], st * k * (1 + 2.0 ** -8 + extra))
    assert float(C.exact_product(1, 256, H, C.C3, None, bias=False)["split"][0, 2]) == 257 + 3 / 1024


@pytest.mark.parametrize("k", KS)
def test_constructs_held_bitwise_on_the_fp32_chains_are_exact_in_any_order(k):
    """With the split off the device test compares bitwise only where the sum of |products| and
    |bias|, over the lowest bit any of them has, is below 2^24: c1 in every column and c2 in one
    chunk are, c2 and c3 in every column are not (those are held in units)."""
    for n in (1, 37, MULTI):
        e = C.exact_product(n, k, H, C.C1, None)
        assert e["span"] < 2.0 ** 24 and torch.equal(e["split"], e["plain"])
        assert C.representable(e["plain"])
        for p in C.chunk_positions(k):
            e = C.exact_product(n, k, H, C.C2, _chunk(p), bias=False)
            assert e["span"] < 2.0 ** 24 and torch.equal(e["split"], e["plain"])
        for c in (C.C2, C.C3):
            assert C.exact_product(n, k, H, c, None)["span"] >= 2.0 ** 24
        # dgrad: reduction over the 128 h
        e = C.exact_product(n, H, k, C.C1, None, bias=False)
        assert e["span"] < 2.0 ** 24 and C.representable(e["plain"])
        for p in (0, 7):
            e = C.exact_product(n, H, k, C.C2, _chunk(p), bias=False)
            assert e["span"] < 2.0 ** 24 and torch.equal(e["split"], e["plain"])


@pytest.mark.parametrize("n", [1, 37, MULTI])
@pytest.mark.parametrize("k", KS)
def test_backward_constructs_give_the_stated_values(k, n):
    for const in ("c2", "c3"):
        c = C.CONSTS[const]
        for cols in (None, _chunk(0), _chunk(7)):
            e = C.exact_product(n, H, k, c, cols, bias=False)
            want = e["split"].float()
            assert C.representable(e["split"])
            assert torch.equal(S.split_matmul(e["a"], e["b"]), want)
            assert torch.equal(_f32(e["a"].double() @ e["b"].double().T), want)
        for cols in [None] + [_chunk(p) for p in C.chunk_positions(k)]:
            e = C.exact_wgrad(n, k, H, c, cols)
            assert C.representable(e["dw_split"]) and C.representable(e["db"])
            dzt, xt = e["dz"].T.contiguous(), e["x"].T.contiguous()
            assert torch.equal(S.split_matmul(dzt, xt, flush=32), e["dw_split"].float())
            assert torch.equal(_f32(dzt.double() @ xt.double().T), e["dw_split"].float())
            assert torch.equal(e["dw_plain"], dzt.double() @ xt.double().T)
            assert torch.equal(e["db"], e["dz"].double().sum(0))
    # where the device test holds dW / db bitwise with the split off, any order of rows is exact
    e = C.exact_wgrad(n, k, H, C.C1)
    assert e["dw_span"] < 2.0 ** 24 and e["db_span"] < 2.0 ** 24
    assert torch.equal(e["dw_split"], e["dw_plain"]) and C.representable(e["dw_plain"])
    if n <= 63:
        assert C.exact_wgrad(n, k, H, C.C2)["dw_span"] < 2.0 ** 24


def test_wgrad_row_weights():
    """At most 63 rows: weight 1 each.  More: powers of two, every 32-row tile (the ragged last
    one too) summing to 64, so the whole sum is 64 m, m <= 63, and m (2^18 + 2^10 + 3) fits
    24 bits."""
    assert C.wgrad_row_weights(37) == [1] * 37
    m = C.wgrad_row_weights(MULTI)
    assert len(m) == MULTI and all(v & (v - 1) == 0 and v > 0 for v in m)
    tiles = [sum(m[r:r + 32]) for r in range(0, MULTI, 32)]
    assert set(tiles) == {64} and len(tiles) <= 63
    assert (len(tiles) * (2 ** 18 + 2 ** 10 + 3)).bit_length() <= 24


# ---------------------------------------------------------------------------- mixed rows
def test_row_scales_are_exact_powers_of_two():
    sc = C.row_scales(MULTI, C.ROW_EXPS)
    assert sorted(set(sc.tolist())) == [2.0 ** e for e in C.ROW_EXPS]
    for r0 in range(0, MULTI - 32, 32):                  # every exponent inside every row tile
        assert len(set(sc[r0:r0 + 32].tolist())) == len(C.ROW_EXPS)
    d = C.draw([512], H, MULTI, rep=200)
    xs = (d["x"].double() * sc[:, None]).float()
    # the emulated split commutes with the row scaling bit for bit (what the device test asks)
    base = S.split_matmul(d["x"], d["w"], flush=256)
    assert torch.equal(S.split_matmul(xs, d["w"], flush=256), _f32(base.double() * sc[:, None]))
