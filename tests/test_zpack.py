"""Zero-packed fp32 rows (``csrc/zpack.h``): the pack pass, the packed dP gather and its wiring in
the link loss.

The contract is bitwise: the packed gather keeps the unpacked kernel's lanes and the order of
every sum, and the format is lossless (a value is stored iff its bit pattern is non-zero), so
every GPU comparison here is ``torch.equal`` against the unpacked path on the same inputs.  The
per-lane address arithmetic is checked on the host by ``tests/host/zpack_check.cpp``, built with
the address and undefined-behaviour sanitizers and run as a program of its own.

Shapes: 300 users, 37 posts, about 3000 positive edges at chunk 64 (posts above and below the
heavy-row threshold, so the slab and the fixup run), one post without positives, one without
negatives; widths 64 and 128.  The user table is a ReLU of normal draws (half zeros) with these
rows forced: all zero, fully dense, 28 / 29 non-zeros (16 + 4 * 28 = 128: the first line
boundary), 60 / 61, one holding -0.0 and a denormal, and the table's last row, which an edge
references."""
import pathlib
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N

ROOT = pathlib.Path(__file__).resolve().parents[1]
N_USERS, N_POSTS = 300, 37
CHUNK = 64
DS = (64, 128)
NO_POS, HEAVY, NO_NEG = 0, 1, 2            # posts
ZERO, DENSE, NNZ28, NNZ29, NNZ60, NNZ61, ODD = range(7)   # user rows
LAST = N_USERS - 1
HGNN_E_ARG, HGNN_E_UNSUPPORTED = 1001, 1004


# ----------------------------------------------------------------------------- CPU
def test_host_check_of_the_lane_arithmetic_under_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "zpack_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "truth_recommendation_gnn_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "zpack_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "zpack_check ok" in r.stdout


def test_slot_stride_and_supported_widths():
    lib = N.lib()
    assert lib.hgnn_zpack_slot_bytes(128) == 640
    assert lib.hgnn_zpack_slot_bytes(64) == 384
    for d in (0, 32, 96, 256):
        assert lib.hgnn_zpack_slot_bytes(d) == 0
    assert lib.hgnn_zpack_rows(None, 5, 96, None, None, None) == HGNN_E_UNSUPPORTED
    assert b"d=96" in lib.hgnn_last_error_string()
    assert lib.hgnn_zpack_rows(None, 5, 128, None, None, None) == HGNN_E_ARG
    assert lib.hgnn_zpack_rows(None, 0, 128, None, None, None) == 0
    assert lib.hgnn_score_gather2_zp(None, 10, None, 96, None, None, None, None, 5, None, 1.0,
                                     None, None, 0, 0, CHUNK, None, None,
                                     None) == HGNN_E_UNSUPPORTED
    assert lib.hgnn_score_gather2_zp(None, 10, None, 128, None, None, None, None, 5, None, 1.0,
                                     None, None, 0, 0, CHUNK, None, None, None) == HGNN_E_ARG


def test_policy(monkeypatch):
    lib = N.lib()
    gib = 1 << 30
    monkeypatch.delenv("HGNN_ZPACK", raising=False)
    assert lib.hgnn_zpack_policy(9_000_000 * 512, 128, 1) == 1      # cfg4's user table
    assert lib.hgnn_zpack_policy(gib, 64, 1) == 1
    assert lib.hgnn_zpack_policy(gib - 1, 128, 1) == 0              # cfg2 / cfg3: cache-resident
    assert lib.hgnn_zpack_policy(9_000_000 * 512, 128, 0) == 0      # a dense table, never
    assert lib.hgnn_zpack_policy(8 * gib, 96, 1) == 0
    monkeypatch.setenv("HGNN_ZPACK", "auto")
    assert lib.hgnn_zpack_policy(9_000_000 * 512, 128, 1) == 1
    assert lib.hgnn_zpack_policy(9_000_000 * 512, 128, 0) == 0
    monkeypatch.setenv("HGNN_ZPACK", "0")
    assert lib.hgnn_zpack_policy(9_000_000 * 512, 128, 1) == 0
    monkeypatch.setenv("HGNN_ZPACK", "1")
    assert lib.hgnn_zpack_policy(1024, 128, 0) == 1
    assert lib.hgnn_zpack_policy(1024, 96, 1) == 0


def test_relu_outputs_are_marked_where_they_are_produced():
    import inspect
    from truth_recommendation_gnn_amd import ops
    for fn in (ops.linear_fwd, ops.linear_fwd_many):
        assert "RELU_OUT" in inspect.getsource(fn)
    t = torch.zeros(2, 2)
    assert not getattr(t, ops.RELU_OUT, False)


# ----------------------------------------------------------------------------- GPU
def _graph():
    rng = np.random.default_rng(11)
    deg = rng.integers(20, 101, N_POSTS)
    deg[NO_POS], deg[HEAVY], deg[NO_NEG] = 0, 700, 40
    post = np.repeat(np.arange(N_POSTS), deg)
    user = rng.integers(0, N_USERS, post.size)
    # every forced row and the last row of the table are read, by a light and by a heavy post
    forced = np.array([ZERO, DENSE, NNZ28, NNZ29, NNZ60, NNZ61, ODD, LAST])
    user = np.concatenate([user, forced, forced])
    post = np.concatenate([post, np.full(8, 5), np.full(8, HEAVY)])
    perm = rng.permutation(post.size)
    user, post = user[perm], post[perm]
    neg = rng.integers(0, N_POSTS, post.size)
    neg[neg == NO_NEG] = NO_NEG + 1
    neg[np.isin(user, forced)] = 7               # the forced rows as negatives too, of one post
    return user, post, neg


def _table(d, seed):
    """fp32 bit patterns [N_USERS, d]: ReLU of normal draws, with the forced rows."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((N_USERS, d)), 0).astype(np.float32)

    def with_nnz(k):
        row = np.zeros(d, np.float32)
        row[rng.permutation(d)[:k]] = (0.25 + rng.random(k)).astype(np.float32)
        return row

    x[ZERO] = 0
    x[DENSE] = (0.25 + rng.random(d)).astype(np.float32)
    for r, k in ((NNZ28, 28), (NNZ29, 29), (NNZ60, 60), (NNZ61, 61)):
        x[r] = with_nnz(k)
    bits = x.view(np.uint32)
    bits[ODD] = 0
    bits[ODD, 3] = 0x80000000                    # -0.0
    bits[ODD, 4] = 0x00000001                    # the smallest denormal
    bits[ODD, d - 1] = 0x00800000 - 1            # the largest denormal
    bits[ODD, 17] = 0x3F800000
    x[LAST] = with_nnz(61)
    x[LAST, d - 1] = 1.5
    x[LAST, 0] = 0
    return x


def _pack_ref(x):
    """numpy reference of the format: per row (mask bytes, value bytes)."""
    n, d = x.shape
    bits = x.view(np.uint32)
    rows = []
    for r in range(n):
        nz = bits[r] != 0
        mask = np.zeros(16, np.uint8)
        mask[:d // 8] = np.packbits(nz, bitorder="little")
        rows.append((mask, bits[r][nz].astype("<u4").view(np.uint8)))
    return rows


@pytest.fixture(scope="module")
def g():
    from truth_recommendation_gnn_amd.graph import NO_SPLIT, GroupedEdges, Plan, RelationCSR
    user, post, neg = _graph()
    dev = torch.device("cuda:0")
    ei_up = torch.from_numpy(np.stack([user, post])).to(dev)
    pos = RelationCSR(ei_up, N_USERS, N_POSTS, chunk=CHUNK).fwd          # posts <- users
    assert pos.plan.n_heavy > 0
    # the negatives grouped by post, as the loss's sort leaves them
    order = np.argsort(neg, kind="stable")
    rowptr_n = np.zeros(N_POSTS + 1, np.int64)
    np.cumsum(np.bincount(neg, minlength=N_POSTS), out=rowptr_n[1:])
    users_n = torch.from_numpy(user[order].astype(np.int32)).to(dev)
    negs = GroupedEdges(torch.from_numpy(rowptr_n.astype(np.int32)).to(dev), users_n, users_n,
                        Plan(NO_SPLIT, 0, 0, None, None), N_POSTS)
    rp = pos.rowptr.cpu().numpy()
    assert rp[NO_POS + 1] == rp[NO_POS] and rp[HEAVY + 1] - rp[HEAVY] > CHUNK
    assert rowptr_n[NO_NEG + 1] == rowptr_n[NO_NEG]
    assert LAST in user
    return types.SimpleNamespace(dev=dev, ei_up=ei_up, pos=pos, negs=negs, E=int(post.size),
                                 neg_edge=torch.from_numpy(neg).to(dev))


_IN = {}


def _inputs(g, d):
    if d not in _IN:
        gen = torch.Generator().manual_seed(300 + d)
        x = _table(d, 400 + d)
        _IN[d] = types.SimpleNamespace(
            x=x, U=torch.from_numpy(x).to(g.dev),
            P=(0.3 * torch.randn(N_POSTS, d, generator=gen)).to(g.dev),
            pw=(0.5 + torch.rand(g.E, generator=gen)).to(g.dev))
    return _IN[d]


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_pack_matches_the_numpy_reference(g, d):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(g, d)
    slot = 640 if d == 128 else 384
    hist = torch.zeros(6, dtype=torch.int64, device=g.dev)
    out = ops.zpack_rows(t.U, hist)
    assert out.dtype == torch.uint8 and out.numel() == N_USERS * slot
    got = out.cpu().numpy().reshape(N_USERS, slot)
    want_hist = np.zeros(6, np.int64)
    for r, (mask, vals) in enumerate(_pack_ref(t.x)):
        assert np.array_equal(got[r, :16], mask), r
        assert np.array_equal(got[r, 16:16 + vals.size], vals), r
        want_hist[(16 + vals.size + 127) // 128] += 1
    assert np.array_equal(hist.cpu().numpy(), want_hist)
    assert want_hist[1] >= 2 and want_hist[2] >= 2     # both sides of the first line boundary
    # the pass adds into hist; without one it writes the same bytes
    again = ops.zpack_rows(t.U).cpu().numpy().reshape(N_USERS, slot)
    for r, (mask, vals) in enumerate(_pack_ref(t.x)):
        assert np.array_equal(again[r, :16 + vals.size], got[r, :16 + vals.size]), r


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_packed_gather_is_bitwise_the_unpacked_gather(g, d):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(g, d)
    c = t.pw.mean()
    want = torch.empty(N_POSTS, d, device=g.dev)
    got = torch.full((N_POSTS, d), float("nan"), device=g.dev)
    ops._score_gather2(t.U, t.P, g.pos, g.negs, c, 1.0 / g.E, want)
    ops._score_gather2(t.U, t.P, g.pos, g.negs, c, 1.0 / g.E, got, ops.zpack_rows(t.U))
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert float(want[HEAVY].abs().max()) > 0 and float(want[NO_POS].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_unwritten_slot_bytes_never_reach_the_result(g, d):
    """The same packed rows laid over a buffer of NaN patterns and over one of zeros."""
    from truth_recommendation_gnn_amd import ops
    t = _inputs(g, d)
    c = t.pw.mean()
    slot = 640 if d == 128 else 384
    ref = _pack_ref(t.x)
    outs = []
    for fill in (0xFF, 0x00):
        buf = np.full((N_USERS, slot), fill, np.uint8)
        for r, (mask, vals) in enumerate(ref):
            buf[r, :16] = mask
            buf[r, 16:16 + vals.size] = vals
        out = torch.empty(N_POSTS, d, device=g.dev)
        ops._score_gather2(t.U, t.P, g.pos, g.negs, c, 1.0 / g.E, out,
                           torch.from_numpy(buf.reshape(-1)).to(g.dev))
        outs.append(out)
    want = torch.empty(N_POSTS, d, device=g.dev)
    ops._score_gather2(t.U, t.P, g.pos, g.negs, c, 1.0 / g.E, want)
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)


def _timed_names(fn):
    from truth_recommendation_gnn_amd import ops
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        res = fn()
    finally:
        ops.set_timer(None)
    return res, [r[0] for r in timer.records]


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_loss_with_packed_rows_is_bitwise_the_loss_without(g, d, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(g, d)
    c = t.pw.mean()

    def run():
        return ops.edge_bce_loss_raw(t.U, t.P, g.ei_up, g.neg_edge, g.E, c, neg_order="edge")

    monkeypatch.setenv("HGNN_ZPACK", "0")
    want, names0 = _timed_names(run)
    monkeypatch.setenv("HGNN_ZPACK", "1")
    got, names1 = _timed_names(run)
    assert not any(n.startswith("zpack[") for n in names0)
    assert f"zpack[{N_USERS}]x{d}" in names1
    gather = f"score_gather[{N_POSTS}<-{N_USERS}]x{d}"
    assert gather in names0 and gather in names1          # the timer entry keeps its name
    for a, b, name in zip(got, want, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name
    # the autograd entry takes the same path and hands the same gradients on
    U, P = t.U.clone().requires_grad_(), t.P.clone().requires_grad_()
    ops.edge_bce_loss(U, P, g.ei_up, g.neg_edge, t.pw, neg_order="edge").backward()
    assert torch.equal(U.grad, want[1]) and torch.equal(P.grad, want[2])


@pytest.mark.gpu
def test_auto_keeps_dense_and_small_tables_unpacked(g, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(g, 128)
    c = t.pw.mean()
    monkeypatch.setenv("HGNN_ZPACK", "auto")
    assert not ops.zpack_on(t.U, False)
    big = torch.empty(3_000_000, 128, device="meta")       # 1.5 GB
    assert not ops.zpack_on(big, False)                    # not a ReLU output: never
    assert ops.zpack_on(big, True)
    assert not ops.zpack_on(torch.empty(3_000_000, 96, device="meta"), True)
    _, names = _timed_names(lambda: ops.edge_bce_loss_raw(
        t.U, t.P, g.ei_up, g.neg_edge, g.E, c, neg_order="edge"))
    assert not any(n.startswith("zpack[") for n in names)
    # a fused-ReLU K3 output carries the mark; at this size auto still leaves it unpacked
    w = torch.randn(128, 128, device=g.dev) / 11
    y = ops.linear_fwd([t.U], w, None, True)
    assert getattr(y, ops.RELU_OUT, False) and float((y == 0).float().mean()) > 0.2
    assert not getattr(ops.linear_fwd([t.U], w, None, False), ops.RELU_OUT, False)
    assert not ops.zpack_on(y, True)
    _, names = _timed_names(lambda: ops.edge_bce_loss_raw(
        y, t.P, g.ei_up, g.neg_edge, g.E, c, neg_order="edge"))
    assert not any(n.startswith("zpack[") for n in names)
