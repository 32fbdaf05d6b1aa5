"""Hot-row flags (``hgnn_hot_cols``) and the two-policy row loads of K1 / K2 / the scoring pass.

The loads change only the cache policy, never the edge order, so every result under
``HGNN_HOT_ROWS=force`` must be bitwise what ``HGNN_HOT_ROWS=0`` gives (``torch.equal``).  The
graph is small (300 destination rows over 50 Zipf-drawn source rows) and holds the rows at which
the kernels change path: an empty row, one of exactly 64 edges and one of 65 (the 64-edge index
chunk), and rows long enough to be split at chunk 64 (heavy-row plan + fixup), one of them above
the ``acc_limit`` used below.  H in {0, 1, 7, 50}: all rows cold, slots of one step holding hot
and cold rows together, all rows hot.

The fused loss is run under both settings too: its scoring pass was measured with the policy and
kept on its old path, so loss, dU and dP must not depend on the switch at all."""
import types

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N

N_DST, N_SRC = 300, 50
CHUNK = 64
ACC_LIMIT = 150
HS = (0, 1, 7, 50)
DS = (128, 64, 20)


def _edges():
    """(src ids, dst rows) on the CPU: fixed degrees for the path-changing rows, Zipf(0.8)-like
    source ids."""
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 13, N_DST)
    deg[0], deg[1], deg[2], deg[3], deg[200] = 0, 64, 65, 700, 300
    dst = np.repeat(np.arange(N_DST), deg)
    p = 1.0 / np.arange(1, N_SRC + 1) ** 0.8
    src = rng.choice(N_SRC, size=dst.size, p=p / p.sum())
    perm = rng.permutation(dst.size)
    return torch.from_numpy(src[perm]), torch.from_numpy(dst[perm])


def _top_h(deg: np.ndarray, h: int) -> np.ndarray:
    """The h most referenced ids, ties to the lower id."""
    order = np.lexsort((np.arange(deg.size), -deg))
    return order[:h]


# ----------------------------------------------------------------------------- CPU
def test_policy_rule_is_off_for_a_small_table(monkeypatch):
    lib = N.lib()
    monkeypatch.delenv("HGNN_HOT_ROWS", raising=False)
    assert lib.hgnn_hot_rows_policy(N_SRC * 128 * 4, 1, 0.9) == 0       # small table
    assert lib.hgnn_hot_rows_policy(1_000_000 * 128 * 4, 1, 0.555) == 1  # cfg4's post table
    assert lib.hgnn_hot_rows_policy(1_000_000 * 128 * 4, 1, 0.346) == 0  # too thin a head
    assert lib.hgnn_hot_rows_policy(1_000_000 * 128 * 4, 1, 0.05) == 0   # uniform ids
    assert lib.hgnn_hot_rows_policy(1_000_000 * 128 * 4, 0, 0.555) == 0  # no col_hot
    monkeypatch.setenv("HGNN_HOT_ROWS", "force")
    assert lib.hgnn_hot_rows_policy(N_SRC * 128 * 4, 1, 0.0) == 1
    assert lib.hgnn_hot_rows_policy(N_SRC * 128 * 4, 0, 1.0) == 0
    monkeypatch.setenv("HGNN_HOT_ROWS", "0")
    assert lib.hgnn_hot_rows_policy(1_000_000 * 128 * 4, 1, 0.555) == 0


def test_an_id_of_2_pow_31_or_more_is_refused():
    from truth_recommendation_gnn_amd import graph
    rc = N.lib().hgnn_hot_cols(None, 2**31 + 1, None, 10, 5, None, None, None, 0, None)
    assert rc != 0
    assert b"2^31" in N.lib().hgnn_last_error_string()
    with pytest.raises(ValueError, match="2\\^31"):
        graph.build_hot_cols(types.SimpleNamespace(col=None), None, 2**31 + 1, 5)


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def rels():
    """The two relations over the same edges: src -> dst (K1 reads the 50-row table through
    ``fwd``) and its flip (K2 and the loss read it through ``bwd``)."""
    from truth_recommendation_gnn_amd.graph import RelationCSR
    src, dst = _edges()
    dev = torch.device("cuda:0")
    ei = torch.stack([src, dst]).to(dev)
    k1 = RelationCSR(ei, N_SRC, N_DST, chunk=CHUNK)
    ei_up = ei.flip(0).contiguous()          # (user, post): K2's relation and the loss's edges
    k2 = RelationCSR(ei_up, N_DST, N_SRC, chunk=CHUNK)
    assert k1.fwd.plan.n_heavy == 3 and k2.bwd.plan.n_heavy == 3   # rows 2, 3 and 200 are split
    return types.SimpleNamespace(ei=ei, ei_up=ei_up, k1=k1, k2=k2, src=src.numpy(),
                                 dst=dst.numpy())


def _inputs(rels, d):
    g = torch.Generator().manual_seed(100 + d)
    dev = torch.device("cuda:0")
    return types.SimpleNamespace(
        x=torch.randn(N_SRC, d, generator=g).to(dev),
        pre=torch.randn(N_DST, d, generator=g).to(dev),
        U=(0.3 * torch.randn(N_DST, d, generator=g)).to(dev),
        neg=torch.randint(0, N_SRC, (rels.src.size,), generator=g).to(dev))


def _raw_k2(rels, x, pre, hot):
    """The weighted K2 through the C entry with ``acc_limit``: rows below it accumulate into
    ``pre``, the others are written fresh."""
    g, p = rels.k2.bwd, rels.k2.bwd.plan
    d = int(x.shape[1])
    out = pre.clone()
    slab = torch.empty(p.n_chunks * d, dtype=torch.float32, device=x.device)
    N.check(N.lib().hgnn_gather_reduce_hot(
        N.ptr(x), N_SRC, d, N.ptr(g.rowptr), N.ptr(g.col), g.n_rows, N.ptr(rels.k2.bwd_weights),
        None, N.HGNN_ACCUMULATE, N.ptr(p.heavy_rows), N.ptr(p.heavy_first), p.n_heavy,
        p.n_chunks, p.chunk, N.ptr(slab), N.ptr(out), ACC_LIMIT,
        N.ptr(hot.col) if hot is not None else None, hot.share if hot is not None else 0.0,
        N.stream_ptr(x.device)), "hgnn_gather_reduce_hot")
    return out


def _run_all(rels, t, d):
    """Every result the policy may touch, as a dict of tensors."""
    from truth_recommendation_gnn_amd import ops
    nbytes = N_SRC * d * 4
    out = {"k1_mean": ops.gather_mean(t.x, rels.k1),
           "k2_fresh": ops.scatter_mean_bwd(t.x, rels.k2),
           "k2_accumulate": ops.scatter_mean_bwd(t.x, rels.k2, out=t.pre.clone()),
           "k2_acc_limit": _raw_k2(rels, t.x, t.pre, rels.k2.hot_cols("bwd", nbytes))}
    c = torch.tensor(0.7, device=t.x.device)
    loss, dU, dP = ops.edge_bce_loss_raw(t.U, t.x, rels.ei_up, t.neg,
                                         int(t.neg.numel()), c, neg_order="edge")
    out.update(loss=loss, dU=dU, dP=dP)
    torch.cuda.synchronize()
    return out


_REF = {}


def _reference(rels, d, monkeypatch):
    """The policy-off results of width d, computed once and shared by the H cases."""
    if d not in _REF:
        monkeypatch.setenv("HGNN_HOT_ROWS", "0")
        assert rels.k1.hot_cols("fwd", N_SRC * d * 4) is None
        _REF[d] = _run_all(rels, _inputs(rels, d), d)
        # acc_limit itself: rows below it hold pre + the fresh sums, the others the fresh sums
        r = _REF[d]
        lo = slice(0, ACC_LIMIT)
        assert torch.equal(r["k2_acc_limit"][ACC_LIMIT:], r["k2_fresh"][ACC_LIMIT:])
        assert torch.equal(r["k2_acc_limit"][lo], r["k2_accumulate"][lo])
    return _REF[d]


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("h", HS)
def test_results_are_bitwise_those_of_the_policy_off(rels, monkeypatch, d, h):
    ref = _reference(rels, d, monkeypatch)
    monkeypatch.setenv("HGNN_HOT_ROWS", "force")
    monkeypatch.setenv("HGNN_HOT_ROWS_H", str(h))
    hc = rels.k1.hot_cols("fwd", N_SRC * d * 4)
    assert hc is not None and hc.h == h                 # the forced policy really has a col_hot
    assert int((hc.col < 0).sum()) == round(hc.share * hc.col.numel())
    assert (h == 0) == (hc.share == 0.0) and (h == N_SRC) == (hc.share == 1.0)
    got = _run_all(rels, _inputs(rels, d), d)
    for name, want in ref.items():
        assert torch.equal(got[name], want), name


@pytest.mark.gpu
@pytest.mark.parametrize("h", HS + (13,))
def test_col_hot_flags_the_top_h_rows(rels, h):
    from truth_recommendation_gnn_amd import graph
    deg = np.bincount(rels.src, minlength=N_SRC)
    for g, opposite in ((rels.k1.fwd, rels.k1.bwd), (rels.k2.bwd, rels.k2.fwd)):
        hc = graph.build_hot_cols(g, opposite.rowptr, N_SRC, h)
        col, col_hot = g.col.cpu().numpy(), hc.col.cpu().numpy()
        assert np.array_equal(col_hot & 0x7FFFFFFF, col)
        want = np.isin(col, _top_h(deg, h))
        assert np.array_equal(col_hot < 0, want)
        assert hc.share == pytest.approx(want.mean(), abs=1e-12)


@pytest.mark.gpu
def test_equal_degrees_go_to_the_lower_id():
    from truth_recommendation_gnn_amd import graph
    from truth_recommendation_gnn_amd.graph import RelationCSR
    deg = np.array([3, 5, 5, 5, 2, 5, 0, 3])
    src = np.repeat(np.arange(deg.size), deg)
    dst = np.arange(src.size) % 4
    ei = torch.from_numpy(np.stack([src, dst])).to("cuda:0")
    csr = RelationCSR(ei, deg.size, 4)
    col = csr.fwd.col.cpu().numpy()
    for h, want in ((1, {1}), (3, {1, 2, 3}), (4, {1, 2, 3, 5}), (5, {0, 1, 2, 3, 5}),
                    (6, {0, 1, 2, 3, 5, 7}), (8, set(range(8))), (99, set(range(8)))):
        hc = graph.build_hot_cols(csr.fwd, csr.bwd.rowptr, deg.size, h)
        flagged = set(col[hc.col.cpu().numpy() < 0].tolist())
        assert flagged == want - {6}, (h, flagged)      # (row 6 has no edge to carry a flag)
