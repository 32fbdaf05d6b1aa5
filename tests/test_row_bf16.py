"""bf16 row storage (``HGNN_ROW_DTYPE=bf16``): the cast, the K1/K2 kernel family and the link loss
over bf16 tables, and the straight-through gradient.

The contract: a result in the mode is what the fp32 path gives on R(T) = T.to(bfloat16).float().
Every comparison here rounds the very tensor the kernel under test receives (never activations
the reference computed itself), so the only difference left is fp32 summation order, held to the
project's fp32 bar ``assert_close(rtol=1e-4, atol=1e-5 * max|ref|)``.  The same bf16 kernel under
two cache policies, or run twice, is bitwise equal.

The graph is the one of test_hot_rows.py, built the same way: 300 destination rows over 50
Zipf-drawn source rows, degrees forced to 0, 64, 65, 700 and 300 at chunk 64 (an empty row, both
sides of the 64-edge index chunk, three heavy rows, one of them above ``acc_limit`` = 150).
Widths: 8 (one 16-B vector per row), 64 and 128 (the product's), 264 (33 vectors: the
past-the-row guards), and 32, 256 and 520 for the remaining rows of the bf16 width table."""
import os
import pathlib
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N

ROOT = pathlib.Path(__file__).resolve().parents[1]
N_DST, N_SRC = 300, 50
CHUNK = 64
ACC_LIMIT = 150
DS = (8, 32, 64, 128, 256, 264, 520)
LOSS_DS = (64, 128)
HGNN_E_ARG, HGNN_E_UNSUPPORTED = 1001, 1004


def _edges():
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 13, N_DST)
    deg[0], deg[1], deg[2], deg[3], deg[200] = 0, 64, 65, 700, 300
    dst = np.repeat(np.arange(N_DST), deg)
    p = 1.0 / np.arange(1, N_SRC + 1) ** 0.8
    src = rng.choice(N_SRC, size=dst.size, p=p / p.sum())
    perm = rng.permutation(dst.size)
    return torch.from_numpy(src[perm]), torch.from_numpy(dst[perm])


def close(got, ref):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5 * scale)


def R(t):
    return t.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------- CPU
def _gather_rc(d, rowptr=None, out=None, n_rows=5):
    return N.lib().hgnn_gather_reduce_bf16(
        None, 10, d, rowptr, None, n_rows, None, None, None, N.HGNN_MEAN, None, None, 0, 0, CHUNK,
        None, out, 0, None, 0.0, None)


def test_cast_of_nothing_is_ok():
    assert N.lib().hgnn_rows_to_bf16(None, 0, None, None) == 0


def test_a_width_that_is_no_multiple_of_8_is_unsupported():
    assert _gather_rc(20) == HGNN_E_UNSUPPORTED
    assert b"d=20" in N.lib().hgnn_last_error_string()
    assert _gather_rc(1032) == HGNN_E_UNSUPPORTED
    assert b"d=1032" in N.lib().hgnn_last_error_string()


def test_null_rowptr_or_out_with_rows_is_an_argument_error():
    assert _gather_rc(64) == HGNN_E_ARG
    assert _gather_rc(64, n_rows=0) == 0          # nothing to do, nothing dereferenced
    lib = N.lib()
    assert lib.hgnn_score_gather2_bf16(None, 10, None, 20, None, None, None, None, 5, None, 1.0,
                                       None, None, 0, 0, CHUNK, None, None,
                                       None) == HGNN_E_UNSUPPORTED
    assert lib.hgnn_score_gather2_bf16(None, 10, None, 64, None, None, None, None, 5, None, 1.0,
                                       None, None, 0, 0, CHUNK, None, None, None) == HGNN_E_ARG
    assert lib.hgnn_edge_score_fwd_bf16(None, None, 64, 5, 5, None, None, None, None, None, 3,
                                        None, None, None, None, None, None) == HGNN_E_ARG


def test_row_dtype_defaults_to_fp32():
    from truth_recommendation_gnn_amd import ops
    assert ops.ROW_DTYPE == os.environ.get("HGNN_ROW_DTYPE", "fp32")
    assert ops.ROW_DTYPES == ("fp32", "bf16")
    assert ops.resolve_row_dtype(None) == ops.ROW_DTYPE
    assert ops.LayerSpec((), ()).row_dtype is None


def test_a_bad_row_dtype_names_both_values():
    env = dict(os.environ, HGNN_ROW_DTYPE="fp16")
    r = subprocess.run([sys.executable, "-c", "import truth_recommendation_gnn_amd"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("ValueError") and "fp32" in last and "bf16" in last
    from truth_recommendation_gnn_amd import ops
    with pytest.raises(ValueError, match="fp32.*bf16"):
        ops.resolve_row_dtype("half")


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def rels():
    from truth_recommendation_gnn_amd.graph import RelationCSR
    src, dst = _edges()
    dev = torch.device("cuda:0")
    ei = torch.stack([src, dst]).to(dev)
    k1 = RelationCSR(ei, N_SRC, N_DST, chunk=CHUNK)
    ei_up = ei.flip(0).contiguous()            # (user, post): the loss's edges
    assert k1.fwd.plan.n_heavy == 3
    g = k1.fwd
    return types.SimpleNamespace(ei=ei, ei_up=ei_up, k1=k1, g=g,
                                 rowptr=g.rowptr.cpu().numpy().astype(np.int64),
                                 col=g.col.cpu().numpy().astype(np.int64))


_IN = {}


def _inputs(rels, d):
    """Inputs of width d and the float64 segment sums of the bf16 table they are checked against,
    computed once and left unchanged."""
    if d not in _IN:
        gen = torch.Generator().manual_seed(200 + d)
        dev = torch.device("cuda:0")
        E = rels.col.size
        t = types.SimpleNamespace(
            x=torch.randn(N_SRC, d, generator=gen).to(dev),
            pre=torch.randn(N_DST, d, generator=gen).to(dev),
            edge_w=(0.5 + torch.rand(E, generator=gen)).to(dev),
            col_w=(0.5 + torch.rand(N_SRC, generator=gen)).to(dev),
            row_w=(0.5 + torch.rand(N_DST, generator=gen)).to(dev))
        from truth_recommendation_gnn_amd import ops
        t.xb = ops.rows_to_bf16(t.x)
        assert t.xb.dtype == torch.bfloat16 and torch.equal(t.xb, t.x.to(torch.bfloat16))
        t.x64 = t.xb.float().double().cpu().numpy()
        _IN[d] = t
    return _IN[d]


def _segment_sum64(rels, x64, edge_w=None, col_w=None):
    rows = x64[rels.col]
    if edge_w is not None:
        rows = rows * edge_w.double().cpu().numpy()[:, None]
    if col_w is not None:
        rows = rows * col_w.double().cpu().numpy()[rels.col][:, None]
    cs = np.concatenate([np.zeros((1, x64.shape[1])), np.cumsum(rows, axis=0)])
    return cs[rels.rowptr[1:]] - cs[rels.rowptr[:-1]]


def _deg(rels):
    return (rels.rowptr[1:] - rels.rowptr[:-1]).astype(np.float64)


def _gather(rels, xb, flags=0, edge_w=None, col_w=None, row_w=None, out=None, acc_limit=0,
            hot=None):
    """hgnn_gather_reduce_bf16 over the 300 <- 50 grouping."""
    g, p = rels.g, rels.g.plan
    d = int(xb.shape[1])
    if out is None:
        out = torch.empty(N_DST, d, dtype=torch.float32, device=xb.device)
    slab = torch.empty(p.n_chunks * d, dtype=torch.float32, device=xb.device)
    N.check(N.lib().hgnn_gather_reduce_bf16(
        N.ptr(xb), N_SRC, d, N.ptr(g.rowptr), N.ptr(g.col), g.n_rows, N.ptr(edge_w),
        N.ptr(col_w), N.ptr(row_w), flags, N.ptr(p.heavy_rows), N.ptr(p.heavy_first), p.n_heavy,
        p.n_chunks, p.chunk, N.ptr(slab), N.ptr(out), acc_limit,
        N.ptr(hot.col) if hot is not None else None, hot.share if hot is not None else 0.0,
        N.stream_ptr(xb.device)), "hgnn_gather_reduce_bf16")
    return out


@pytest.mark.gpu
def test_cast_is_bitwise_torchs():
    from truth_recommendation_gnn_amd import ops
    gen = torch.Generator().manual_seed(5)
    big = torch.finfo(torch.float32).max
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -0.0, 0.0,
                            1e-40, -1e-40, 2.0 ** -149, 2.0 ** -133 * 1.00390625,
                            float("inf"), -float("inf"), big, -big, 3.3895e38])
    for n in (1003, 1003 + special.numel(), 8, 1, 4096):
        x = torch.randn(n, generator=gen) * torch.exp(4 * torch.randn(n, generator=gen))
        if n == 1003 + special.numel():
            x[1003:] = special
        x = x.to("cuda:0")
        got = ops.rows_to_bf16(x)
        assert got.dtype == torch.bfloat16 and got.shape == x.shape
        assert torch.equal(got.view(torch.int16), x.to(torch.bfloat16).view(torch.int16)), n
    nan = ops.rows_to_bf16(torch.tensor([float("nan"), 1.0, -float("nan")], device="cuda:0"))
    assert bool(torch.isnan(nan[0])) and bool(torch.isnan(nan[2])) and float(nan[1]) == 1.0
    assert ops.rows_to_bf16(torch.empty(0, 8, device="cuda:0")).shape == (0, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_gather_family_over_a_bf16_table(rels, d):
    t = _inputs(rels, d)
    deg = _deg(rels)
    inv = np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)[:, None]
    plain = _segment_sum64(rels, t.x64)
    pre64 = t.pre.double().cpu().numpy()
    # the mean (empty row -> 0)
    mean = _gather(rels, t.xb, N.HGNN_MEAN)
    close(mean, plain * inv)
    assert float(mean[0].abs().max()) == 0.0
    # the plain sum with edge weights; column weights; both; a per-row scale
    close(_gather(rels, t.xb, edge_w=t.edge_w), _segment_sum64(rels, t.x64, t.edge_w))
    close(_gather(rels, t.xb, col_w=t.col_w), _segment_sum64(rels, t.x64, None, t.col_w))
    close(_gather(rels, t.xb, edge_w=t.edge_w, col_w=t.col_w),
          _segment_sum64(rels, t.x64, t.edge_w, t.col_w))
    close(_gather(rels, t.xb, row_w=t.row_w), plain * t.row_w.double().cpu().numpy()[:, None])
    # accumulate into a non-zero output
    close(_gather(rels, t.xb, N.HGNN_MEAN | N.HGNN_ACCUMULATE, out=t.pre.clone()),
          pre64 + plain * inv)
    # acc_limit: rows below it accumulate, the others (pre-filled with NaN) are overwritten
    out = t.pre.clone()
    out[ACC_LIMIT:] = float("nan")
    got = _gather(rels, t.xb, N.HGNN_ACCUMULATE, out=out, acc_limit=ACC_LIMIT)
    want = plain.copy()
    want[:ACC_LIMIT] += pre64[:ACC_LIMIT]
    assert not bool(torch.isnan(got).any())
    close(got, want)
    # twice the same bits
    assert torch.equal(_gather(rels, t.xb, N.HGNN_MEAN), mean)
    assert torch.equal(_gather(rels, t.xb, edge_w=t.edge_w), _gather(rels, t.xb, edge_w=t.edge_w))


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_gather_mean_takes_a_bf16_table(rels, d, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(rels, d)
    deg = _deg(rels)
    want = _segment_sum64(rels, t.x64) * np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)[:, None]
    monkeypatch.setenv("HGNN_HOT_ROWS", "0")
    one = ops.gather_mean(t.xb, rels.k1)
    assert one.dtype == torch.float32
    close(one, want)
    close(ops.gather_mean(t.xb, rels.k1, out=t.pre.clone()), t.pre.double().cpu().numpy() + want)
    with pytest.raises(ValueError, match="static"):
        ops.gather_mean(t.xb, rels.k1, static=True)
    # the source-blocked path, as 3 passes over thirds of the bf16 table
    nbytes = N_SRC * d * 2
    monkeypatch.setattr(ops, "GATHER_BLOCK_BYTES", 1)
    monkeypatch.setattr(ops, "GATHER_BLOCK_SLICE", -(-nbytes // 3))
    assert ops.gather_blocks(t.xb, rels.k1.num_edges) == 3
    blocked = ops.gather_mean(t.xb, rels.k1)
    close(blocked, want)
    close(ops.gather_mean(t.xb, rels.k1, out=t.pre.clone()), t.pre.double().cpu().numpy() + want)
    assert torch.equal(ops.gather_mean(t.xb, rels.k1), blocked)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("h", (0, 7, 50))
def test_hot_rows_change_no_bit_of_the_bf16_gather(rels, d, h, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(rels, d)
    nbytes = N_SRC * d * 2
    monkeypatch.setenv("HGNN_HOT_ROWS", "0")
    assert rels.k1.hot_cols("fwd", nbytes) is None
    off = ops.gather_mean(t.xb, rels.k1)
    off_w = _gather(rels, t.xb, edge_w=t.edge_w, col_w=t.col_w)
    monkeypatch.setenv("HGNN_HOT_ROWS", "force")
    monkeypatch.setenv("HGNN_HOT_ROWS_H", str(h))
    hc = rels.k1.hot_cols("fwd", nbytes)
    assert hc is not None and hc.h == h
    assert torch.equal(ops.gather_mean(t.xb, rels.k1), off)
    assert torch.equal(_gather(rels, t.xb, N.HGNN_MEAN, hot=hc), off)
    assert torch.equal(_gather(rels, t.xb, edge_w=t.edge_w, col_w=t.col_w, hot=hc), off_w)


# ----------------------------------------------------------------------------- the loss
def _loss_inputs(rels, d):
    gen = torch.Generator().manual_seed(300 + d)
    dev = torch.device("cuda:0")
    E = int(rels.ei_up.shape[1])
    return types.SimpleNamespace(
        U=(0.3 * torch.randn(N_DST, d, generator=gen)).to(dev),
        P=(0.3 * torch.randn(N_SRC, d, generator=gen)).to(dev),
        pw=(0.5 + torch.rand(E, generator=gen)).to(dev),
        neg64=torch.randint(0, N_SRC, (E,), generator=gen).to(dev),
        neg32=torch.randint(0, N_SRC, (E,), generator=gen, dtype=torch.int32).to(dev), E=E)


def _negatives(rels, t, form):
    from truth_recommendation_gnn_amd import ops
    if form == "int64":
        return t.neg64, "edge"
    if form == "int32":
        return t.neg32, "user"
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    return ops.draw_negatives(rels.ei_up, N_SRC, generator=gen), "user"


@pytest.mark.gpu
@pytest.mark.parametrize("d", LOSS_DS)
@pytest.mark.parametrize("form", ("int64", "int32", "draw"))
def test_loss_on_bf16_rows_is_the_fp32_loss_on_the_rounded_tables(rels, d, form):
    from truth_recommendation_gnn_amd import ops
    t = _loss_inputs(rels, d)
    neg, order = _negatives(rels, t, form)
    c = t.pw.mean()
    got = ops.edge_bce_loss_raw(t.U, t.P, rels.ei_up, neg, t.E, c, neg_order=order,
                                row_dtype="bf16")
    ref = ops.edge_bce_loss_raw(R(t.U), R(t.P), rels.ei_up, neg, t.E, c, neg_order=order)
    for a, b, name in zip(got, ref, ("loss", "dU", "dP")):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        close(a, b)
    again = ops.edge_bce_loss_raw(t.U, t.P, rels.ei_up, neg, t.E, c, neg_order=order,
                                  row_dtype="bf16")
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    if form == "draw":      # the draws are hgnn_uniform_i32's
        ref2 = ops.edge_bce_loss_raw(R(t.U), R(t.P), rels.ei_up, neg.tensor(), t.E, c,
                                     neg_order="user")
        for a, b in zip(got, ref2):
            close(a, b)
    if form == "int64":     # and the reference loss itself, float64 autograd on R(U), R(P)
        U64 = R(t.U).double().requires_grad_()
        P64 = R(t.P).double().requires_grad_()
        l64 = ops.link_loss(U64, P64, rels.ei_up, t.neg64, t.pw.double())
        l64.backward()
        close(got[0], l64)
        close(got[1], U64.grad)
        close(got[2], P64.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("d", LOSS_DS)
def test_dp_gather_splits_heavy_posts_on_bf16_rows(rels, d):
    """The loss's own grouping has no row above its chunk at this size, so the dP gather's
    heavy-row plan (slab + fixup) is run here on the same edges at chunk 64."""
    from truth_recommendation_gnn_amd import ops
    from truth_recommendation_gnn_amd.graph import NO_SPLIT, GroupedEdges, Plan, RelationCSR
    t = _loss_inputs(rels, d)
    dev = t.U.device
    pos = RelationCSR(rels.ei_up, N_DST, N_SRC, chunk=CHUNK).fwd     # posts <- users
    assert pos.plan.n_heavy > 0
    none = torch.empty(0, dtype=torch.int32, device=dev)
    negs = GroupedEdges(torch.zeros(N_SRC + 1, dtype=torch.int32, device=dev), none, none,
                        Plan(NO_SPLIT, 0, 0, None, None), N_SRC)
    c = t.pw.mean()
    got = torch.empty(N_SRC, d, device=dev)
    ref = torch.empty(N_SRC, d, device=dev)
    ops._score_gather2(ops.rows_to_bf16(t.U), ops.rows_to_bf16(t.P), pos, negs, c, 1.0 / t.E, got)
    ops._score_gather2(R(t.U), R(t.P), pos, negs, c, 1.0 / t.E, ref)
    close(got, ref)


@pytest.mark.gpu
def test_loss_default_of_the_raw_entry_stays_fp32(rels, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _loss_inputs(rels, 64)
    c = t.pw.mean()
    want = ops.edge_bce_loss_raw(t.U, t.P, rels.ei_up, t.neg32, t.E, c)
    monkeypatch.setattr(ops, "ROW_DTYPE", "bf16")
    got = ops.edge_bce_loss_raw(t.U, t.P, rels.ei_up, t.neg32, t.E, c)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    for kw in ({"ready": lambda: None}, {"on_dP": lambda dP: None},
               {"p_chunks": [(0, N_SRC, None)]}):
        with pytest.raises(ValueError, match="bf16"):
            ops.edge_bce_loss_raw(t.U, t.P, rels.ei_up, t.neg32, t.E, c, row_dtype="bf16", **kw)


@pytest.mark.gpu
def test_loss_autograd_on_bf16_rows(rels, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _loss_inputs(rels, 128)
    c = t.pw.mean()
    _, dU, dP = ops.edge_bce_loss_raw(t.U, t.P, rels.ei_up, t.neg64, t.E, c, neg_order="edge",
                                      row_dtype="bf16")
    U, P = t.U.clone().requires_grad_(), t.P.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, rels.ei_up, t.neg64, t.pw, row_dtype="bf16")
    loss.backward(retain_graph=True)
    g1 = (U.grad.clone(), P.grad.clone())
    assert torch.equal(g1[0], dU) and torch.equal(g1[1], dP)
    U.grad = P.grad = None
    loss.backward()               # the retained graph: recomputed from the saved bf16 shadows
    assert torch.equal(U.grad, g1[0]) and torch.equal(P.grad, g1[1])
    # None is ops.ROW_DTYPE at call time; an explicit "fp32" is the default path whatever it says
    fp32 = ops.edge_bce_loss(t.U, t.P, rels.ei_up, t.neg64, t.pw)
    monkeypatch.setattr(ops, "ROW_DTYPE", "bf16")
    assert torch.equal(ops.edge_bce_loss(t.U, t.P, rels.ei_up, t.neg64, t.pw), loss.detach())
    assert torch.equal(ops.edge_bce_loss(t.U, t.P, rels.ei_up, t.neg64, t.pw, row_dtype="fp32"),
                       fp32)
    assert not torch.equal(fp32, loss.detach())
    # an out-of-range negative is the fp32 path's error
    bad = t.neg64.clone()
    bad[3] = N_SRC
    with pytest.raises(ValueError, match="out of range"):
        ops.edge_bce_loss(t.U, t.P, rels.ei_up, bad, t.pw, row_dtype="bf16")
    monkeypatch.setattr(ops, "ROW_DTYPE", "fp32")
    with pytest.raises(ValueError, match="out of range"):
        ops.edge_bce_loss(t.U, t.P, rels.ei_up, bad, t.pw)


# ----------------------------------------------------------------------------- straight through
@pytest.mark.gpu
@pytest.mark.parametrize("d", (64, 20))
def test_mean_gather_gradient_passes_straight_through(rels, d):
    from truth_recommendation_gnn_amd import ops
    gen = torch.Generator().manual_seed(400 + d)
    x = torch.randn(N_SRC, d, generator=gen).to("cuda:0")
    up = torch.randn(N_DST, d, generator=gen).to("cuda:0")
    grads, outs = [], []
    for mode in ("bf16", "fp32", None):
        xi = x.clone().requires_grad_()
        y = ops.mean_gather(xi, rels.k1, row_dtype=mode)
        y.backward(up)
        grads.append(xi.grad)
        outs.append(y.detach())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[1], grads[2])   # the same K2
    assert torch.equal(outs[1], outs[2])
    if d % 8 == 0:
        assert torch.equal(outs[0], ops.gather_mean(ops.rows_to_bf16(x), rels.k1))
        assert not torch.equal(outs[0], outs[1])
    else:                       # such a width keeps fp32 rows
        assert torch.equal(outs[0], outs[1])
