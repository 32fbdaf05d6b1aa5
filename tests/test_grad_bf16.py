"""bf16 gradient rows (``HGNN_GRAD_ROW_DTYPE=bf16``): the switch, the ReLU-backward cast
``hgnn_relu_grad_to_bf16`` and the K2 scatter over a bf16 gradient table.

The contract: with the mode on, a K2 gives what the fp32 K2 gives on R(T) = T.to(bfloat16).float(),
T being the very fp32 table it would have read; the only difference left is fp32 summation order,
held to the project's fp32 bar ``assert_close(rtol=1e-4, atol=1e-5 * max|ref|)``.  The masked cast
is bitwise ``rows_to_bf16`` of the ``dz_out`` the K3 backward writes.

The graph is the one of test_row_bf16.py: 300 users over 50 Zipf-drawn posts, user degrees forced
to 0, 64, 65, 700 and 300; K2 runs over its CSC (posts <- users), where the Zipf head posts
exceed the 64-edge chunk (heavy rows).  Widths: 8 (one 16-B vector per row), 64 and 128 (the
product's), 264 (33 vectors: the past-the-row guards)."""
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
DS = (8, 64, 128, 264)
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


# ----------------------------------------------------------------------------- CPU: the entry
# No pointer is dereferenced before the checks pass, so made-up addresses stand in for buffers;
# no call here passes every check (that would launch).
A, B, C = 0x10000, 0x20000, 0x30000            # 16-byte aligned


def _rc(dout, out_act, mask, n_rows, h, dz):
    return N.lib().hgnn_relu_grad_to_bf16(dout, out_act, mask, n_rows, h, dz, None)


def _err():
    return N.lib().hgnn_last_error_string().decode()


def test_relu_cast_of_nothing_is_ok_with_null_pointers():
    assert _rc(None, None, None, 0, 64, None) == 0
    assert _rc(None, None, None, 0, 8, None) == 0


def test_relu_cast_width_must_be_a_multiple_of_8():
    assert _rc(A, B, None, 5, 20, C) == HGNN_E_UNSUPPORTED
    assert "relu_grad_to_bf16" in _err() and "h=20" in _err()
    assert _rc(A, B, None, 0, 12, C) == HGNN_E_UNSUPPORTED     # also with no rows
    assert _rc(A, B, None, 5, 0, C) == HGNN_E_UNSUPPORTED


def test_relu_cast_takes_exactly_one_predicate_source():
    assert _rc(A, B, C, 5, 64, A) == HGNN_E_ARG
    assert "relu_grad_to_bf16: both out_act and mask" in _err()
    assert _rc(A, None, None, 5, 64, C) == HGNN_E_ARG
    assert "relu_grad_to_bf16: neither out_act nor mask" in _err()


def test_relu_cast_null_pointer_with_rows_is_an_argument_error():
    for dout, dz in ((None, C), (A, None)):
        assert _rc(dout, B, None, 5, 64, dz) == HGNN_E_ARG
        assert _err() == "relu_grad_to_bf16: null pointer"
        assert _rc(dout, None, B, 5, 64, dz) == HGNN_E_ARG
        assert _err() == "relu_grad_to_bf16: null pointer"
    assert _rc(A, B, None, -1, 64, C) == HGNN_E_ARG
    assert "n_rows=-1" in _err()


def test_relu_cast_pointers_must_be_16_byte_aligned():
    for args in ((A + 8, B, None, C), (A, B + 4, None, C), (A, None, B + 8, C),
                 (A, B, None, C + 2)):
        dout, act, mask, dz = args
        assert _rc(dout, act, mask, 5, 64, dz) == HGNN_E_ARG
        assert "relu_grad_to_bf16" in _err() and "16-byte aligned" in _err()


def test_relu_cast_bit_form_exists_only_where_relu_mask_for_gives_one():
    from truth_recommendation_gnn_amd import ops
    for h in (8, 24, 72, 136, 144, 264):
        assert ops.relu_mask_for(3, h, True, "meta") is None
        assert _rc(A, None, B, 5, h, C) == HGNN_E_UNSUPPORTED
        assert f"h={h}" in _err() and "out_act" in _err()
    for h in range(16, 129, 16):
        assert ops.relu_mask_for(3, h, True, "meta").shape == (3, 4)


# ----------------------------------------------------------------------------- CPU: the switch
def test_grad_row_dtype_defaults_to_fp32():
    env = {k: v for k, v in os.environ.items() if k != "HGNN_GRAD_ROW_DTYPE"}
    code = ("from truth_recommendation_gnn_amd import ops; "
            "print(ops.GRAD_ROW_DTYPE, ops.resolve_grad_row_dtype(None), "
            "ops.LayerSpec((), ()).grad_row_dtype)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["fp32", "fp32", "None"]
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT,
                       env=dict(env, HGNN_GRAD_ROW_DTYPE="bf16", HGNN_ROW_DTYPE="fp32"),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["bf16", "bf16", "None"]


def test_a_bad_grad_row_dtype_names_both_values(monkeypatch):
    env = dict(os.environ, HGNN_GRAD_ROW_DTYPE="fp16")
    r = subprocess.run([sys.executable, "-c", "import truth_recommendation_gnn_amd"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("ValueError") and "HGNN_GRAD_ROW_DTYPE" in last
    assert "fp32" in last and "bf16" in last
    from truth_recommendation_gnn_amd import HeteroSAGE, WeightedRGCN, WeightedRGCNAuthor, ops
    with pytest.raises(ValueError, match="grad_row_dtype.*fp32.*bf16"):
        ops.resolve_grad_row_dtype("half")
    assert ops.resolve_grad_row_dtype("bf16") == "bf16"
    monkeypatch.setattr(ops, "GRAD_ROW_DTYPE", "bf16")      # None: the module value at call time
    assert ops.resolve_grad_row_dtype(None) == "bf16"
    assert ops.resolve_grad_row_dtype("fp32") == "fp32"
    assert ops.resolve_row_dtype(None) == ops.ROW_DTYPE     # the two switches are independent
    rels = [(("user", "engages", "post"), 1.0)]
    for make in (lambda **kw: HeteroSAGE(8, rels, in_channels=8, **kw),
                 lambda **kw: WeightedRGCN(8, **kw), lambda **kw: WeightedRGCNAuthor(8, **kw)):
        with pytest.raises(ValueError, match="grad_row_dtype.*fp32.*bf16"):
            make(grad_row_dtype="half")
        assert make(grad_row_dtype="bf16").grad_row_dtype == "bf16"
        assert make().grad_row_dtype is None


# ----------------------------------------------------------------------------- CPU: the plan
class _Rel:
    def __init__(self, n_src, n_dst, num_edges=7):
        self.n_src, self.n_dst, self.num_edges = n_src, n_dst, num_edges


NU, NP, D, H = 300, 40, 64, 64
SHAPES = {"user": (NU, D), "post": (NP, D)}
PU, UU, UP = _Rel(NP, NU), _Rel(NU, NU), _Rel(NU, NP)   # user<-post, user<-user, post<-user


def _plan(groups, shapes=SHAPES, bf16=False, hidden=None, types_=("post", "user"), **kw):
    from truth_recommendation_gnn_amd import ops
    return ops._layer_plan(ops.LayerSpec(types_, tuple(groups)), shapes,
                           [H] * len(groups) if hidden is None else hidden, bf16, **kw)


def _full(pre_user=(), pu=PU):
    from truth_recommendation_gnn_amd import ops
    return (ops.DstGroup("user", (("post", pu), ("user", UU)), True, True, pre_user),
            ops.DstGroup("post", (("user", UP),), True, True))


def test_plan_marks_every_relation_with_edges_on_full_tables():
    plan = _plan(_full(), grad_bf16=True)
    assert [p.gbf16 for p in plan.groups] == [(True, True), (True,)]
    assert [p.bf16 for p in plan.groups] == [(False, False), (False,)] and plan.shadow == ()
    # a relation without edges runs no K2
    plan = _plan(_full(pu=_Rel(NP, NU, 0)), grad_bf16=True)
    assert [p.gbf16 for p in plan.groups] == [(False, True), (True,)]
    # the two modes are independent
    plan = _plan(_full(), bf16=True, grad_bf16=True)
    assert [p.gbf16 for p in plan.groups] == [(True, True), (True,)]
    assert [p.bf16 for p in plan.groups] == [(True, True), (True,)]


def test_plan_marks_nothing_in_a_sampled_block():
    from truth_recommendation_gnn_amd import ops
    block = (ops.DstGroup("user", (("post", _Rel(NP, 100)), ("user", _Rel(NU, 100))), True, True,
                          (), n_root=100),
             ops.DstGroup("post", (("user", _Rel(NU, 20)),), True, True, (), n_root=20))
    plan = _plan(block, grad_bf16=True)
    assert [p.gbf16 for p in plan.groups] == [(False, False), (False,)]
    g = ops.DstGroup("user", (("post", _Rel(NP, 100)),), True, True, (), None,
                     root_src="user@root")
    plan = _plan((g,), dict(SHAPES, **{"user@root": (100, D)}),
                 types_=("post", "user", "user@root"), grad_bf16=True)
    assert plan.groups[0].gbf16 == (False,)


def test_plan_marks_nothing_at_a_width_that_is_no_multiple_of_8():
    plan = _plan(_full(), {"user": (NU, 20), "post": (NP, 20)}, grad_bf16=True)
    assert [p.gbf16 for p in plan.groups] == [(False, False), (False,)]
    # dA has its own segment's width: the 64-wide post segment is rounded, the 20-wide ones not
    plan = _plan(_full(), {"user": (NU, 20), "post": (NP, 64)}, grad_bf16=True)
    assert [p.gbf16 for p in plan.groups] == [(True, False), (False,)]


def test_plan_judges_a_pre_projected_relation_at_the_output_width():
    # dz is as wide as the group's output: a 20-wide source under a 64-wide output is rounded,
    # a 64-wide source under a 20-wide output is not
    plan = _plan(_full(pre_user=(True, False)), {"user": (NU, 64), "post": (NP, 20)},
                 hidden=[64, 64], grad_bf16=True)
    assert plan.groups[0].gbf16 == (True, True)
    plan = _plan(_full(pre_user=(True, False)), {"user": (NU, 64), "post": (NP, 64)},
                 hidden=[20, 64], grad_bf16=True)
    assert plan.groups[0].gbf16 == (False, True) and plan.groups[1].gbf16 == (True,)


def test_plan_without_the_mode_marks_nothing_and_is_otherwise_the_same():
    for groups, kw in ((_full(), {}), (_full(pre_user=(True, False)), {}),
                       (_full(), {"bf16": True})):
        off = _plan(groups, **kw)                       # four positional arguments, as before
        explicit = _plan(groups, grad_bf16=False, **kw)
        on = _plan(groups, grad_bf16=True, **kw)
        assert off == explicit
        assert all(not any(p.gbf16) for p in off.groups)
        assert all(len(p.gbf16) == len(p.rels) for p in off.groups)
        assert (off.types, off.batched, off.shadow) == (on.types, on.batched, on.shadow)
        for a, b in zip(off.groups, on.groups):
            assert a._replace(gbf16=b.gbf16) == b       # every other field equal


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def rels():
    from truth_recommendation_gnn_amd.graph import RelationCSR
    src, dst = _edges()
    dev = torch.device("cuda:0")
    ei = torch.stack([src, dst]).to(dev)
    k1 = RelationCSR(ei, N_SRC, N_DST, chunk=CHUNK)      # users <- posts; K2 over its CSC
    assert k1.bwd.plan.n_heavy > 0                       # the Zipf head posts exceed the chunk
    return types.SimpleNamespace(ei=ei, k1=k1)


_IN = {}


def _inputs(d):
    """The gradient table of width d, its bf16 copy and the fp32 K2 references, computed once and
    left unchanged."""
    if d not in _IN:
        gen = torch.Generator().manual_seed(500 + d)
        dev = torch.device("cuda:0")
        _IN[d] = types.SimpleNamespace(g=torch.randn(N_DST, d, generator=gen).to(dev),
                                       pre=torch.randn(N_SRC, d, generator=gen).to(dev))
    return _IN[d]


def _specials():
    """±0, denormals and bf16 ties (the patterns of test_row_bf16.test_cast_is_bitwise_torchs)."""
    return torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -0.0, 0.0,
                         1e-40, -1e-40, 2.0 ** -149, 2.0 ** -133 * 1.00390625])


@pytest.mark.gpu
@pytest.mark.parametrize("h", (64, 128, 8, 72, 264))
@pytest.mark.parametrize("n", (1, 7, 300))
def test_masked_cast_is_bitwise_the_two_step_path(n, h):
    from truth_recommendation_gnn_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000 * h + n)
    k = 64 if h in (64, 128) else 24
    x = torch.randn(n, k, generator=gen).to(dev)
    w = (0.3 * torch.randn(h, k, generator=gen)).to(dev)
    b = (0.1 * torch.randn(h, generator=gen)).to(dev)
    add = torch.zeros(n, h)
    add[0] = -1e3                                        # a row that is all masked
    if n > 1:
        add[1] = 1e3                                     # and one with nothing masked
    bits = ops.relu_mask_for(n, h, True, dev)
    assert (bits is not None) == (h in (64, 128))
    y = ops.linear_fwd([x], w, b, True, add=add.to(dev), mask_out=bits)
    assert float(y[0].max()) == 0.0 and (n == 1 or float(y[1].min()) > 0.0)
    if n > 2:
        frac = float((y[2:] > 0).float().mean())
        assert 0.2 < frac < 0.8                          # the other rows are mixed
    # dout: wide-ranged values with the special patterns over every row kind, kept and masked
    dout = torch.randn(n, h, generator=gen) * torch.exp(4 * torch.randn(n, h, generator=gen))
    sp = _specials()
    flat = dout.view(-1)
    pos = torch.randperm(flat.numel(), generator=gen)[:max(flat.numel() // 2, 1)]
    flat[pos] = sp[torch.arange(pos.numel()) % sp.numel()]
    dout = dout.to(dev)

    dz = torch.full((n, h), float("nan"), device=dev)
    dx = torch.empty_like(x)
    ops.linear_bwd([x], w, dout, y, [dx], False, False, dz_out=dz, mask=bits)
    assert torch.equal(dz, torch.where(y > 0, dout, torch.zeros_like(dout)))
    want = ops.rows_to_bf16(dz).view(torch.int16)
    got = ops.relu_grad_bf16(dout, out_act=y)
    assert got.dtype == torch.bfloat16 and got.shape == (n, h)
    assert torch.equal(got.view(torch.int16), want)
    if bits is not None:
        assert torch.equal(ops.relu_grad_bf16(dout, mask=bits).view(torch.int16), want)
        with pytest.raises(N.NativeError, match="both out_act and mask"):
            ops.relu_grad_bf16(dout, out_act=y, mask=bits)
    with pytest.raises(N.NativeError, match="neither out_act nor mask"):
        ops.relu_grad_bf16(dout)


@pytest.mark.gpu
def test_masked_cast_of_no_rows():
    from truth_recommendation_gnn_amd import ops
    dev = torch.device("cuda:0")
    e = torch.empty(0, 64, device=dev)
    assert ops.relu_grad_bf16(e, out_act=e).shape == (0, 64)
    assert ops.relu_grad_bf16(e, mask=torch.empty(0, 4, dtype=torch.int32, device=dev)).shape \
        == (0, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_scatter_mean_bwd_takes_a_bf16_table(rels, d, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(d)
    monkeypatch.setenv("HGNN_HOT_ROWS", "0")
    gb = ops.rows_to_bf16(t.g)
    want = ops.scatter_mean_bwd(R(t.g), rels.k1)
    one = ops.scatter_mean_bwd(gb, rels.k1)
    assert one.dtype == torch.float32 and one.shape == (N_SRC, d)
    close(one, want)
    want_acc = ops.scatter_mean_bwd(R(t.g), rels.k1, out=t.pre.clone())
    close(ops.scatter_mean_bwd(gb, rels.k1, out=t.pre.clone()), want_acc)
    assert torch.equal(ops.scatter_mean_bwd(gb, rels.k1), one)          # twice the same bits
    # the source-blocked path, as 3 passes over thirds of the bf16 table
    nbytes = N_DST * d * 2
    monkeypatch.setattr(ops, "GATHER_BLOCK_BYTES", 1)
    monkeypatch.setattr(ops, "GATHER_BLOCK_SLICE", -(-nbytes // 3))
    assert ops.gather_blocks(gb, rels.k1.num_edges) == 3
    blocked = ops.scatter_mean_bwd(gb, rels.k1)
    close(blocked, want)
    close(ops.scatter_mean_bwd(gb, rels.k1, out=t.pre.clone()), want_acc)
    assert torch.equal(ops.scatter_mean_bwd(gb, rels.k1), blocked)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("h", (0, 7, 50))
def test_hot_rows_change_no_bit_of_the_bf16_scatter(rels, d, h, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    t = _inputs(d)
    gb = ops.rows_to_bf16(t.g)
    nbytes = N_DST * d * 2
    monkeypatch.setenv("HGNN_HOT_ROWS", "0")
    assert rels.k1.hot_cols("bwd", nbytes) is None
    off = ops.scatter_mean_bwd(gb, rels.k1)
    off_acc = ops.scatter_mean_bwd(gb, rels.k1, out=t.pre.clone())
    monkeypatch.setenv("HGNN_HOT_ROWS", "force")
    monkeypatch.setenv("HGNN_HOT_ROWS_H", str(h))
    hc = rels.k1.hot_cols("bwd", nbytes)
    assert hc is not None and hc.h == h
    assert torch.equal(ops.scatter_mean_bwd(gb, rels.k1), off)
    assert torch.equal(ops.scatter_mean_bwd(gb, rels.k1, out=t.pre.clone()), off_acc)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_rounding_error_of_the_scatter_is_within_the_derived_bound(rels, d):
    """bf16 keeps 8 significant bits, so |R(x) - x| <= 2^-8 |x| for normal x, and K2's weights
    (1 / deg) are non-negative: elementwise |K2(R(g)) - K2(g)| <= 2^-8 K2(|g|), plus the fp32
    bar's atol for the summation order."""
    from truth_recommendation_gnn_amd import ops
    t = _inputs(d)
    exact = ops.scatter_mean_bwd(t.g, rels.k1)
    mag = ops.scatter_mean_bwd(t.g.abs(), rels.k1)
    got = ops.scatter_mean_bwd(ops.rows_to_bf16(t.g), rels.k1)
    bound = 2.0 ** -8 * mag.double() + 1e-5 * float(exact.abs().max())
    err = (got.double() - exact.double()).abs()
    print(f"d={d}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert not torch.equal(got, exact)                   # the mode does something
