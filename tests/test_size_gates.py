"""The kernel paths that a table's byte size selects, and rows past element 2^31.

Several launchers choose another template instantiation, or another runtime branch, from the size
of a table ("Size gates").  Each rule is one host function that its launcher
calls and that is exported as a probe: ``hgnn_score_nt_policy``, ``hgnn_gather_nt_policy``,
``hgnn_loss_one_pass``, ``hgnn_zpack_policy``, ``hgnn_hot_rows_policy``.  The CPU tests pin every
rule one row below its threshold and at it.  Every GPU case takes its row count FROM the probe
(the smallest count at which it turns on) and asserts through the probe which side of the gate it
runs on, so a retuned threshold fails here instead of leaving a test that checks nothing.

Construction (the embedded graph).  The small graphs the suite already trusts -- the loss graph,
tables, weights and ``[E, k]`` negatives of ``tests/test_loss_multi_neg.py`` and the 300 x 50
gather graph of ``tests/test_hot_rows.py`` (an empty row, the 64 / 65-edge rows, three heavy
rows), both copied -- have their ids relabelled by a strictly increasing map into ``[0, N)``: the
first id goes to 0, the last to N - 1, ids 1 and n - 2 to 1 and N - 2 (so two mapped rows share
one block of four waves at either end) and the others to a seeded sorted sample.  The big tables
are zeros with the base rows written at the mapped positions; negatives are explicit ids.  An
increasing map keeps the order of the COO edges, of every CSR's columns, of the stable sorts and
of the heavy rows' chunks, so the arithmetic of a row does not depend on the table's size:

* loss, gradient rows and output rows at the mapped positions against float64 (autograd of
  ``_ref64``'s expression; float64 segment sums) on the BASE graph at the project's bar, rtol
  1e-4 and atol 1e-5 of the reference's largest entry; bf16 rows against tables rounded to bf16;
* the same rows bitwise (``torch.equal``) against the small-table GPU run of the same case, which
  differs in cache policy only (the loss value is not bitwise: its block partials group
  differently);
* every unmapped row exactly zero, or exactly the prior ``out`` under accumulate, checked on the
  device over the whole complement.

``test_the_embedding_preserves_*`` check the construction itself in plain torch on the CPU.

Rows past element 2^31: N = 2^24 + 8 rows at d = 128, whose last 8 rows lie past element index
2^31.  Those cases need tens of GiB; each works out its need and skips only when
``torch.cuda.mem_get_info()`` shows less free memory than that."""
import contextlib
import ctypes
import gc
import os
import types

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N
from truth_recommendation_gnn_amd import ops

RTOL, ATOL_SCALE = 1e-4, 1e-5
MIB, GIB = 1 << 20, 1 << 30
HGNN_E_ARG = 1001
BCE = torch.nn.functional.binary_cross_entropy_with_logits
MODES = ((1, "mean"), (1, "edge"), (3, "mean"), (3, "edge"))      # (negatives per edge, weighting)
N31, D31 = (1 << 24) + 8, 128                                     # rows past element 2^31


def close(got, ref, rtol=RTOL, atol_scale=ATOL_SCALE):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6)
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol_scale * scale)


# ----------------------------------------------------------------------------- the probes
def score_nt(n_posts, d, bf16=False):
    return int(N.lib().hgnn_score_nt_policy(int(n_posts), int(d), 1 if bf16 else 0))


def gather_nt(n_x, d, elem_bytes, score, n_rows):
    """(nt_load, nt_store) of a gather launch."""
    load, store = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = N.lib().hgnn_gather_nt_policy(int(n_x), int(d), int(elem_bytes), 1 if score else 0,
                                       int(n_rows), ctypes.byref(load), ctypes.byref(store))
    assert rc == 0, N.lib().hgnn_last_error_string()
    return load.value, store.value


def one_pass(n_users):
    return int(N.lib().hgnn_loss_one_pass(int(n_users)))


def smallest(pred, hi=1 << 40):
    """The smallest n >= 1 with pred(n), for a rule that is monotone in n: bisection on the probe."""
    lo = 0
    assert pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


def posts_above_nt_neg(d, bf16=False):
    return smallest(lambda n: score_nt(n, d, bf16))


def users_above_nt_load(d, elem_bytes):
    return smallest(lambda n: gather_nt(n, d, elem_bytes, True, 1)[0])


def rows_above_nt_store(d):
    return smallest(lambda n: gather_nt(1, d, 4, False, n)[1])


@contextlib.contextmanager
def env(**kv):
    """Environment variables set (a string) or removed (None) for the block; the policies read
    them per call."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ----------------------------------------------------------------------------- the id maps
def idmap(n, n_big, seed):
    """A strictly increasing map of ids 0 .. n - 1 into [0, n_big): int64 numpy array."""
    assert n >= 4 and n_big >= n
    if n_big == n:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    mid = np.sort(rng.choice(n_big - 4, size=n - 4, replace=False)) + 2       # in [2, n_big - 2)
    m = np.concatenate([[0, 1], mid, [n_big - 2, n_big - 1]]).astype(np.int64)
    assert (np.diff(m) > 0).all() and m[0] == 0 and m[-1] == n_big - 1
    return m


# ----------------------------------------------------------------------------- the loss graph
# (tests/test_loss_multi_neg.py: _graph, _tables, _negatives, _weights, _ref64 -- copied)
N_USERS, N_POSTS = 300, 37
BIG_USER, NO_EDGE_USER = 0, 1
NO_POS, HEAVY, NO_NEG = 0, 1, 2            # posts
ONLY_LAST = NO_POS


def _graph():
    rng = np.random.default_rng(23)
    deg = rng.integers(40, 121, N_POSTS)
    deg[NO_POS], deg[HEAVY] = 0, 200
    post = np.repeat(np.arange(N_POSTS), deg)
    user = rng.integers(2, N_USERS, post.size)             # users 0 and 1 are placed by hand
    big = rng.integers(3, N_POSTS, 130)                    # 130 positives of one user
    user = np.concatenate([user, np.full(130, BIG_USER)])
    post = np.concatenate([post, big])
    perm = rng.permutation(post.size)
    user, post = user[perm], post[perm]
    neg = rng.integers(0, N_POSTS, post.size)
    neg[neg == NO_NEG] = NO_NEG + 1
    assert (user == BIG_USER).sum() == 130 and not (user == NO_EDGE_USER).any()
    assert (post == HEAVY).sum() == 200 and not (post == NO_POS).any()
    assert not (neg == NO_NEG).any() and 2800 <= post.size <= 3400
    return user, post, neg


def _tables(d, relu=False):
    gen = torch.Generator().manual_seed(500 + d)
    U = 0.3 * torch.randn(N_USERS, d, generator=gen)
    P = 0.3 * torch.randn(N_POSTS, d, generator=gen)
    if relu:
        U = torch.relu(U) * 1.5                            # half zeros, as a fused-ReLU output
    return U, P


def _negatives(E, k):
    """[E, k] int64 in COO order: NO_NEG nowhere, ONLY_LAST in column k - 1 and in no other."""
    rng = np.random.default_rng(100 + k)
    neg = rng.integers(0, N_POSTS, (E, k))
    neg[neg == NO_NEG] = NO_NEG + 1
    head = neg[:, :k - 1]
    head[head == ONLY_LAST] = HEAVY
    neg[::7, k - 1] = ONLY_LAST
    return torch.from_numpy(neg)


def _scores64(U, P, ei):
    return (U.double()[ei[0]] * P.double()[ei[1]]).sum(1)


def _weights(U, P, ei):
    s = _scores64(U, P, ei)
    return torch.where(s < s.median(), 3.0, 1.0).float()


def _ref64(U, P, ei, neg, w, weighting):
    """float64 autograd of the loss written out: (loss, dU, dP) for a unit upstream gradient."""
    Ur, Pr = U.double().requires_grad_(), P.double().requires_grad_()
    u = Ur[ei[0]]
    sp = (u * Pr[ei[1]]).sum(1)
    sn = (u[:, None, :] * Pr[neg]).sum(-1) if neg.dim() == 2 else (u * Pr[neg]).sum(1)
    neg_loss = BCE(sn, torch.zeros_like(sn))               # the mean over all E k
    if weighting == "edge":
        loss = (w.double() * BCE(sp, torch.ones_like(sp), reduction="none")).mean() + neg_loss
    else:
        loss = (w.double() * BCE(sp, torch.ones_like(sp))).mean() + neg_loss
    loss.backward()
    return loss.detach(), Ur.grad, Pr.grad


_LOSS = {}


def loss_graph():
    """The base loss graph on the CPU, built once: edges and the negatives of k = 1 and k = 3."""
    if "g" not in _LOSS:
        user, post, neg1 = _graph()
        ei = torch.from_numpy(np.stack([user, post]))
        E = int(ei.shape[1])
        _LOSS["g"] = types.SimpleNamespace(ei=ei, E=E, neg={1: torch.from_numpy(neg1),
                                                             3: _negatives(E, 3)})
    return _LOSS["g"]


def loss_inputs(d, kind):
    """Base tables of one width and row format (``fp32``, ``bf16``, ``zp``: post-ReLU fp32), their
    weights, and the float64 references per mode: built once, never written.  ``U`` / ``P`` are
    what the kernels get (bf16 tensors for ``bf16``), ``Ur`` / ``Pr`` what the reference reads
    (the same values in fp32)."""
    key = (d, kind)
    if key not in _LOSS:
        g = loss_graph()
        U, P = _tables(d, relu=kind == "zp")
        if kind == "bf16":
            U, P = U.to(torch.bfloat16), P.to(torch.bfloat16)
        Ur, Pr = U.float(), P.float()
        _LOSS[key] = types.SimpleNamespace(U=U, P=P, Ur=Ur, Pr=Pr, w=_weights(Ur, Pr, g.ei),
                                           ref={}, small={})
    return _LOSS[key]


def loss_ref(t, k, weighting):
    if (k, weighting) not in t.ref:
        g = loss_graph()
        t.ref[k, weighting] = _ref64(t.Ur, t.Pr, g.ei, g.neg[k], t.w, weighting)
    return t.ref[k, weighting]


# ----------------------------------------------------------------------------- the gather graph
# (tests/test_hot_rows.py: _edges -- copied)
N_DST, N_SRC = 300, 50
CHUNK = 64
ACC_LIMIT = 150
PRIOR = 0.25                               # the unmapped rows of an `out` that is accumulated into


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


def seg_mean64(src, dst, x, n_dst, w=None, mean=True):
    """float64: out[i] = (mean or sum) over edges (j -> i) of w_e x[j]."""
    v = x.double()[src]
    if w is not None:
        v = v * w.double()[:, None]
    out = torch.zeros(n_dst, x.shape[1], dtype=torch.float64).index_add_(0, dst, v)
    if mean:
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).double()[:, None]
    return out


def k2_ref64(src, dst, x):
    """float64 K2 of the flipped relation: out[row] = sum over edges (row, id) of x[id] / cnt[id],
    cnt the number of edges that reference id."""
    cnt = torch.bincount(src, minlength=x.shape[0]).double()
    return seg_mean64(src, dst, x, N_DST, w=1.0 / cnt[src], mean=False)


# ----------------------------------------------------------------------------- CPU: the rules
@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("d", (64, 128, 200, 5, 260, 264))
def test_score_nt_rule_at_its_threshold(d, bf16):
    row = d * (2 if bf16 else 4)
    n = -(-256 * MIB // row)                               # the first row count of >= 256 MiB
    assert n * row >= 256 * MIB > (n - 1) * row
    assert score_nt(n, d, bf16) == 1 and score_nt(n - 1, d, bf16) == 0
    assert posts_above_nt_neg(d, bf16) == n
    assert score_nt(0, d, bf16) == 0 and score_nt(37, d, bf16) == 0


@pytest.mark.parametrize("elem", (4, 2))
@pytest.mark.parametrize("d", (128, 64, 200, 20))
def test_gather_nt_rule_at_its_thresholds(d, elem):
    n = -(-GIB // (d * elem))
    # a score gather: loads and stores follow the SOURCE table's bytes in its stored dtype,
    # whatever the number of output rows
    for n_rows in (1, 37, 1 << 30):
        assert gather_nt(n, d, elem, True, n_rows) == (1, 1)
        assert gather_nt(n - 1, d, elem, True, n_rows) == (0, 0)
    assert users_above_nt_load(d, elem) == n
    # K1 / K2: never nt loads; nt stores by the fp32 OUTPUT's bytes, whatever the source
    m = -(-GIB // (d * 4))
    for n_x in (1, 50, 1 << 30):
        assert gather_nt(n_x, d, elem, False, m) == (0, 1)
        assert gather_nt(n_x, d, elem, False, m - 1) == (0, 0)
    assert rows_above_nt_store(d) == m


def test_gather_nt_rule_checks_its_arguments():
    lib = N.lib()
    a, b = ctypes.c_int32(7), ctypes.c_int32(7)
    ok = (10, 64, 4, 0, 10, ctypes.byref(a), ctypes.byref(b))
    assert lib.hgnn_gather_nt_policy(*ok) == 0 and (a.value, b.value) == (0, 0)
    for i, bad in ((0, -1), (1, 0), (2, 3), (2, 8), (4, -1), (5, None), (6, None)):
        args = list(ok)
        args[i] = bad
        assert lib.hgnn_gather_nt_policy(*args) == HGNN_E_ARG, i
        assert b"gather_nt_policy" in lib.hgnn_last_error_string()


def test_loss_one_pass_rule_at_its_threshold():
    # 65536 block partials of four users each
    assert one_pass(4 * 65536) == 1 and one_pass(4 * 65536 + 1) == 0
    assert one_pass(0) == 1 and one_pass(300) == 1 and one_pass(9_000_000) == 0
    assert smallest(lambda n: not one_pass(n)) == 4 * 65536 + 1


def test_zpack_and_hot_rows_rules_at_their_thresholds():
    lib = N.lib()
    with env(HGNN_ZPACK=None, HGNN_HOT_ROWS=None):
        for d in (64, 128):
            n = -(-GIB // (4 * d))
            assert lib.hgnn_zpack_policy(n * 4 * d, d, 1) == 1
            assert lib.hgnn_zpack_policy((n - 1) * 4 * d, d, 1) == 0
            assert lib.hgnn_zpack_policy(n * 4 * d, d, 0) == 0
            m = -(-256 * MIB // (4 * d))
            assert lib.hgnn_hot_rows_policy(m * 4 * d, 1, 0.5) == 1
            assert lib.hgnn_hot_rows_policy((m - 1) * 4 * d, 1, 0.5) == 0
            assert lib.hgnn_hot_rows_policy(m * 4 * d, 1, 0.499) == 0


# ----------------------------------------------------------------------------- CPU: the embedding
def test_idmap_is_increasing_with_the_ends_and_adjacent_rows():
    for n, n_big, seed in ((300, 4000, 1), (37, 5000, 2), (50, 64, 3), (300, N31, 4)):
        m = idmap(n, n_big, seed)
        assert m.shape == (n,) and (np.diff(m) > 0).all()
        assert m[0] == 0 and m[-1] == n_big - 1
        assert m[1] // 4 == m[0] // 4                       # two mapped rows in one 4-wave block
        assert m[-1] - m[-2] == 1
        assert np.array_equal(m, idmap(n, n_big, seed))
    assert np.array_equal(idmap(300, 300, 9), np.arange(300))
    assert idmap(300, N31, 4)[-1] * D31 >= 2**31                # the last rows lie past 2^31


def test_the_embedding_preserves_the_loss_and_its_gradients():
    g = loss_graph()
    nu, np_, d = 4000, 3001, 8
    mu, mp = torch.from_numpy(idmap(N_USERS, nu, 11)), torch.from_numpy(idmap(N_POSTS, np_, 12))
    ei_big = torch.stack([mu[g.ei[0]], mp[g.ei[1]]])
    # the order of a stable sort by either endpoint is the base graph's
    for r in (0, 1):
        assert np.array_equal(np.argsort(ei_big[r].numpy(), kind="stable"),
                              np.argsort(g.ei[r].numpy(), kind="stable"))
    U, P = (t.double() for t in _tables(d))
    w = _weights(U, P, g.ei).double()
    for k, weighting in MODES:
        neg = g.neg[k]
        Ub, Pb = torch.zeros(nu, d, dtype=torch.float64), torch.zeros(np_, d, dtype=torch.float64)
        Ub[mu], Pb[mp] = U, P
        Ub.requires_grad_(), Pb.requires_grad_()
        Us, Ps = U.clone().requires_grad_(), P.clone().requires_grad_()
        big = ops.link_loss(Ub, Pb, ei_big, mp[neg], w, weighting=weighting)
        small = ops.link_loss(Us, Ps, g.ei, neg, w, weighting=weighting)
        assert torch.equal(big.detach(), small.detach()), (k, weighting)
        ref = _ref64(U.clone(), P.clone(), g.ei, neg, w, weighting)   # (it marks its inputs)
        assert abs(float(small.detach()) - float(ref[0])) <= 1e-12 * abs(float(ref[0]))
        big.backward()
        small.backward()
        for gb, gs, m, r in ((Ub.grad, Us.grad, mu, ref[1]), (Pb.grad, Ps.grad, mp, ref[2])):
            torch.testing.assert_close(gb[m], gs, rtol=1e-12, atol=1e-15)
            torch.testing.assert_close(gs, r, rtol=1e-12, atol=1e-15)
            assert int(torch.count_nonzero(gb)) == int(torch.count_nonzero(gb[m])) > 0


def test_the_embedding_preserves_the_segment_sums():
    src, dst = _edges()
    n_big, d = 3000, 8
    md, ms = torch.from_numpy(idmap(N_DST, n_big, 13)), torch.from_numpy(idmap(N_SRC, n_big, 14))
    x = torch.randn(N_SRC, d, generator=torch.Generator().manual_seed(5)).double()
    base = seg_mean64(src, dst, x, N_DST)
    # destinations embedded
    big = seg_mean64(src, md[dst], x, n_big)
    assert torch.equal(big[md], base)
    assert int(torch.count_nonzero(big)) == int(torch.count_nonzero(base)) > 0
    # sources embedded
    xb = torch.zeros(n_big, d, dtype=torch.float64).index_copy_(0, ms, x)
    assert torch.equal(seg_mean64(ms[src], dst, xb, N_DST), base)
    # K2 of the flipped relation, its output rows embedded
    k2 = k2_ref64(src, dst, x)
    cnt = torch.bincount(src, minlength=N_SRC).double()
    k2_big = seg_mean64(src, md[dst], x, n_big, w=1.0 / cnt[src], mean=False)
    assert torch.equal(k2_big[md], k2)
    assert int(torch.count_nonzero(k2_big)) == int(torch.count_nonzero(k2))


# ----------------------------------------------------------------------------- GPU: helpers
_LIVE = []                                 # the big fixtures' holders: at most one has contents


def _release():
    """Free whatever an earlier big fixture still holds, then the allocator's cache."""
    from truth_recommendation_gnn_amd import graph
    for h in _LIVE:
        h.__dict__.clear()
    del _LIVE[:]
    graph.CSR_CACHE._d.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _holder(**kw):
    h = types.SimpleNamespace(**kw)
    _LIVE.append(h)
    return h


@pytest.fixture(scope="module", autouse=True)
def _free_at_the_end():
    yield
    _release()


def dev():
    return torch.device("cuda:0")


def embed(base, m, n, fill=0.0):
    """[n, d] on the device: ``fill`` everywhere, the base rows at the mapped positions ``m``."""
    if fill == 0.0:
        big = torch.zeros(n, base.shape[1], dtype=base.dtype, device=dev())
    else:
        big = torch.full((n, base.shape[1]), fill, dtype=base.dtype, device=dev())
    big[m] = base.to(dev())
    return big


def only_mapped_rows_are_written(big, m, fill=0.0):
    """Whether every row of ``big`` outside ``m`` is exactly ``fill``: one pass on the device.
    (Overwrites the mapped rows: take them first.)"""
    big[m] = fill
    if fill == 0.0:
        return int(torch.count_nonzero(big)) == 0
    return bool((big == fill).all())


def require_free(need_bytes):
    free, _ = torch.cuda.mem_get_info()
    if free < need_bytes:
        pytest.skip(f"needs {need_bytes / GIB:.1f} GiB of free device memory, "
                    f"{free / GIB:.1f} GiB are free")


def run_loss(ei_d, U, P, neg_d, w_d, weighting):
    """(loss, dU, dP) for a unit upstream gradient, from the fused kernels outside autograd."""
    if weighting == "edge":
        return ops.edge_bce_loss_raw(U, P, ei_d, neg_d, None, None, neg_order="edge",
                                     pos_weights=w_d, weighting="edge")
    return ops.edge_bce_loss_raw(U, P, ei_d, neg_d, int(ei_d.shape[1]), w_d.mean(),
                                 neg_order="edge")


def small_loss(t, kind, k, weighting):
    """The small-table GPU run of one mode (the zero-packed case packs its 300 rows too, so only
    the nt policy differs from the big run); kept on the CPU."""
    if (k, weighting) not in t.small:
        g = loss_graph()
        U = t.U.to(dev())
        if kind == "zp":
            setattr(U, ops.RELU_OUT, True)
        with env(HGNN_ZPACK="1" if kind == "zp" else "0", HGNN_HOT_ROWS=None):
            out = run_loss(g.ei.to(dev()), U, t.P.to(dev()), g.neg[k].to(dev()), t.w.to(dev()),
                           weighting)
        t.small[k, weighting] = tuple(o.cpu() for o in out)
    return t.small[k, weighting]


def embedded_loss_case(d, kind, n_users, n_posts):
    """The loss graph with its users and posts embedded into ``n_users`` x ``n_posts`` rows."""
    _release()
    g, t = loss_graph(), loss_inputs(d, kind)
    mu = torch.from_numpy(idmap(N_USERS, n_users, 100 + d)).to(dev())
    mp = torch.from_numpy(idmap(N_POSTS, n_posts, 200 + d)).to(dev())
    ei = g.ei.to(dev())
    U = embed(t.U, mu, n_users)
    if kind == "zp":
        setattr(U, ops.RELU_OUT, True)
    return _holder(d=d, kind=kind, t=t, mu=mu, mp=mp, U=U, P=embed(t.P, mp, n_posts),
                   ei=torch.stack([mu[ei[0]], mp[ei[1]]]).contiguous(), w=t.w.to(dev()),
                   neg={k: mp[v.to(dev())].contiguous() for k, v in g.neg.items()},
                   n_users=n_users, n_posts=n_posts)


def check_loss_mode(c, k, weighting, tag):
    """One mode of an embedded case: float64 on the base graph, the small run bitwise, and the
    unmapped rows."""
    ref, small = loss_ref(c.t, k, weighting), small_loss(c.t, c.kind, k, weighting)
    with env(HGNN_ZPACK=None, HGNN_HOT_ROWS=None):
        loss, dU, dP = run_loss(c.ei, c.U, c.P, c.neg[k], c.w, weighting)
    rows = (("dU", dU, c.mu, ref[1], small[1]), ("dP", dP, c.mp, ref[2], small[2]))
    print(tag, c.d, c.kind, k, weighting, "loss", float(loss), float(ref[0]), float(small[0]))
    close(loss, ref[0])
    for name, big, m, r, s in rows:
        got = big[m].cpu()
        print(tag, c.d, c.kind, k, weighting, name, float((got.double() - r).abs().max()),
              float(r.abs().max()))
        close(got, r)
        assert torch.equal(got, s), (name, "differs from the small-table run")
        assert float(got.abs().max()) > 0
        assert only_mapped_rows_are_written(big, m), (name, "an unmapped row is not zero")
    del loss, dU, dP


def elem_of(kind):
    return 2 if kind == "bf16" else 4


# ----------------------------------------------------------------------------- GPU: scoring pass
SCORE_CASES = [(d, "fp32") for d in (64, 128, 200, 5, 260)] + \
              [(d, "bf16") for d in (64, 128, 200, 264)]


@pytest.fixture(scope="module", params=SCORE_CASES, ids=lambda p: f"{p[1]}-d{p[0]}")
def score_case(request):
    """Posts embedded at the smallest row count above the nt_neg gate; the 300 users as they are."""
    d, kind = request.param
    n_posts = posts_above_nt_neg(d, kind == "bf16")
    c = embedded_loss_case(d, kind, N_USERS, n_posts)
    yield c
    _release()


@pytest.mark.gpu
@pytest.mark.parametrize("k,weighting", MODES)
def test_scoring_pass_above_nt_neg(score_case, k, weighting):
    """``k_edge_score<.., NT=true, ..>`` / ``k_edge_score_k<.., NT=true, ..>``, plain and EW."""
    c = score_case
    bf16 = c.kind == "bf16"
    assert score_nt(c.n_posts, c.d, bf16) == 1 and score_nt(c.n_posts - 1, c.d, bf16) == 0
    assert score_nt(N_POSTS, c.d, bf16) == 0                 # the small run: the other side
    assert gather_nt(N_USERS, c.d, elem_of(c.kind), True, c.n_posts) == (0, 0)
    assert one_pass(N_USERS) == 1
    assert tuple(c.P.shape) == (c.n_posts, c.d) and c.P.element_size() == elem_of(c.kind)
    check_loss_mode(c, k, weighting, "score")


# ----------------------------------------------------------------------------- GPU: dP gather
DP_CASES = [(128, "fp32"), (64, "fp32"), (200, "fp32"), (128, "bf16"), (64, "bf16"),
            (128, "zp"), (64, "zp")]


@pytest.fixture(scope="module", params=DP_CASES, ids=lambda p: f"{p[1]}-d{p[0]}")
def dp_case(request):
    """Users embedded at the smallest row count above the 1-GiB gate of the score gathers, posts
    at the nt_neg size."""
    d, kind = request.param
    n_users = users_above_nt_load(d, elem_of(kind))
    n_posts = posts_above_nt_neg(d, kind == "bf16")
    c = embedded_loss_case(d, kind, n_users, n_posts)
    yield c
    _release()


@pytest.mark.gpu
@pytest.mark.parametrize("k,weighting", MODES)
def test_dp_gather_above_the_1_gib_gate(dp_case, k, weighting):
    """The ``SC && a.nt_load`` loads and ``nt_store`` of ``hgnn_score_gather2*`` (fp32, bf16), the
    ``k_gather_zp<.., ZP=2>`` forms, plain and EW; with more than 262144 users also
    ``k_loss_partial`` + ``k_loss_final``, and the scoring pass above nt_neg once more."""
    c = dp_case
    e, lib = elem_of(c.kind), N.lib()
    assert gather_nt(c.n_users, c.d, e, True, c.n_posts) == (1, 1)
    assert gather_nt(c.n_users - 1, c.d, e, True, c.n_posts) == (0, 0)
    assert gather_nt(N_USERS, c.d, e, True, N_POSTS) == (0, 0)   # the small run
    assert score_nt(c.n_posts, c.d, c.kind == "bf16") == 1
    assert one_pass(c.n_users) == 0 and one_pass(N_USERS) == 1
    assert c.U.numel() * c.U.element_size() == c.n_users * c.d * e
    with env(HGNN_ZPACK=None):
        packed = ops.zpack_on(c.U, bool(getattr(c.U, ops.RELU_OUT, False)))
        assert packed == (c.kind == "zp")                        # `auto`, no env: the mark alone
        if c.kind == "zp":
            assert lib.hgnn_zpack_policy((c.n_users - 1) * c.d * 4, c.d, 1) == 0
            assert 0.3 < float((c.t.U == 0).float().mean()) < 0.7
    check_loss_mode(c, k, weighting, "dP")


# ----------------------------------------------------------------------------- GPU: loss reduction
@pytest.mark.gpu
def test_loss_reduction_on_both_sides_of_its_gate():
    """``k_loss_one`` at the largest user count it takes, ``k_loss_partial`` + ``k_loss_final``
    one user above."""
    d = 8
    n_two = smallest(lambda n: not one_pass(n))
    for n_users, want in ((n_two - 1, 1), (n_two, 0)):
        assert one_pass(n_users) == want
        c = embedded_loss_case(d, "fp32", n_users, N_POSTS)
        assert score_nt(N_POSTS, d) == 0 and gather_nt(n_users, d, 4, True, N_POSTS) == (0, 0)
        for k, weighting in MODES:
            check_loss_mode(c, k, weighting, f"reduce[{n_users}]")
    _release()


# ----------------------------------------------------------------------------- GPU: mean gathers
def _raw_k2(k2, x, out, acc_limit, hot):
    """The weighted K2 through the C entry with ``acc_limit``: rows below it accumulate into
    ``out``, the others are written fresh (tests/test_hot_rows.py)."""
    g, p = k2.bwd, k2.bwd.plan
    d = int(x.shape[1])
    slab = torch.empty(p.n_chunks * d, dtype=torch.float32, device=x.device)
    N.check(N.lib().hgnn_gather_reduce_hot(
        N.ptr(x), x.shape[0], d, N.ptr(g.rowptr), N.ptr(g.col), g.n_rows, N.ptr(k2.bwd_weights),
        None, N.HGNN_ACCUMULATE, N.ptr(p.heavy_rows), N.ptr(p.heavy_first), p.n_heavy,
        p.n_chunks, p.chunk, N.ptr(slab), N.ptr(out), acc_limit,
        N.ptr(hot.col) if hot is not None else None, hot.share if hot is not None else 0.0,
        N.stream_ptr(x.device)), "hgnn_gather_reduce_hot")
    return out


# name -> (runner(c, k1, k2, prior, acc_limit), reference key, what the unmapped rows hold)
VARIANTS = {
    "k1_mean": (lambda c, k1, k2, prior, lim: ops.gather_mean(c.x, k1), "mean", "zero"),
    "k1_mean_out": (lambda c, k1, k2, prior, lim: ops.gather_mean(c.x, k1, out=prior()),
                    "mean+pre", "prior"),
    "k1_weighted": (lambda c, k1, k2, prior, lim: ops.weighted_gather_raw(c.x, k1, c.w_pos),
                    "wsum", "zero"),
    "k1_bf16": (lambda c, k1, k2, prior, lim: ops.gather_mean(c.xb, k1), "mean_bf16", "zero"),
    "k2_fresh": (lambda c, k1, k2, prior, lim: ops.scatter_mean_bwd(c.x, k2), "k2", "zero"),
    "k2_accumulate": (lambda c, k1, k2, prior, lim: ops.scatter_mean_bwd(c.x, k2, out=prior()),
                      "k2+pre", "prior"),
    "k2_acc_limit": (lambda c, k1, k2, prior, lim: _raw_k2(
        k2, c.x, prior(), lim, k2.hot_cols("bwd", c.x.numel() * 4)), "k2+pre_lim", "limit"),
}
HOT_VARIANTS = ("k1_mean", "k1_mean_out", "k1_bf16", "k2_fresh", "k2_accumulate", "k2_acc_limit")


def gather_inputs(d):
    """Tables, weights and float64 references of the 300 x 50 gather graph at one width (CPU)."""
    src, dst = _edges()
    gen = torch.Generator().manual_seed(100 + d)
    x, x2 = torch.randn(N_SRC, d, generator=gen), torch.randn(N_SRC, d, generator=gen)
    pre = torch.randn(N_DST, d, generator=gen)
    w_edge = 0.5 + torch.rand(src.numel(), generator=gen)
    xb = x.to(torch.bfloat16) if d % 8 == 0 else None
    mean, k2 = seg_mean64(src, dst, x, N_DST), k2_ref64(src, dst, x)
    lim = torch.arange(N_DST)[:, None] < ACC_LIMIT
    ref = {"mean": mean, "mean+pre": mean + pre.double(), "mean2": seg_mean64(src, dst, x2, N_DST),
           "wsum": seg_mean64(src, dst, x, N_DST, w=w_edge, mean=False),
           "k2": k2, "k2+pre": k2 + pre.double(), "k2+pre_lim": k2 + pre.double() * lim}
    if xb is not None:
        ref["mean_bf16"] = seg_mean64(src, dst, xb.float(), N_DST)
    return types.SimpleNamespace(src=src, dst=dst, x=x, x2=x2, xb=xb, pre=pre, w_edge=w_edge,
                                 ref=ref)


def relations(src_ids, dst_ids, n_src, n_dst, chunk=CHUNK):
    """(ei, its flip, K1's relation src -> dst, K2's relation of the flipped edges): the edge
    tensors are returned too, the relations hold them weakly."""
    from truth_recommendation_gnn_amd.graph import RelationCSR
    ei = torch.stack([src_ids, dst_ids]).to(dev()).contiguous()
    ei_up = ei.flip(0).contiguous()
    return ei, ei_up, RelationCSR(ei, n_src, n_dst, chunk=chunk), \
        RelationCSR(ei_up, n_dst, n_src, chunk=chunk)


def build_mean_case(d):
    """The gather graph with its 300 destination rows embedded at the smallest row count whose
    fp32 output has 1 GiB, beside the same graph as it is."""
    _release()
    b = gather_inputs(d)
    n_big = rows_above_nt_store(d)
    md = torch.from_numpy(idmap(N_DST, n_big, 300 + d))
    small, big = relations(b.src, b.dst, N_SRC, N_DST), relations(b.src, md[b.dst], N_SRC, n_big)
    for s, g in ((small[2].fwd, big[2].fwd), (small[3].bwd, big[3].bwd)):
        assert s.plan.n_heavy == g.plan.n_heavy == 3 and torch.equal(s.perm, g.perm)
        assert torch.equal(s.col, g.col)                      # the 50 source ids, in the same order
    c = _holder(d=d, b=b, n_big=n_big, md=md.to(dev()), small=small, big=big, x=b.x.to(dev()),
                x2=b.x2.to(dev()), xb=b.xb.to(dev()) if b.xb is not None else None,
                pre=b.pre.to(dev()), w_pos=b.w_edge.to(dev())[small[2].fwd.perm.long()].contiguous(),
                ref=b.ref, kept={})
    return c


@pytest.fixture(scope="module", params=(128, 64), ids=lambda d: f"d{d}")
def mean_case(request):
    yield build_mean_case(request.param)
    _release()


def _mean_run(c, name, side):
    run = VARIANTS[name][0]
    if side == "small":
        return run(c, c.small[2], c.small[3], lambda: c.pre.clone(), ACC_LIMIT)
    return run(c, c.big[2], c.big[3], lambda: embed(c.pre, c.md, c.n_big, fill=PRIOR),
               int(c.md[ACC_LIMIT]))


def _small_mean(c, name):
    """The small run with the hot-row policy off: the result every other setting must repeat."""
    if name not in c.kept:
        with env(HGNN_HOT_ROWS="0"):
            c.kept[name] = _mean_run(c, name, "small")
    return c.kept[name]


def _check_mean_variant(c, name, hot):
    d, (_, ref_key, rest) = c.d, VARIANTS[name]
    assert gather_nt(N_SRC, d, 2 if name == "k1_bf16" else 4, False, c.n_big) == (0, 1)
    assert gather_nt(N_SRC, d, 4, False, c.n_big - 1) == (0, 0)
    assert gather_nt(N_SRC, d, 4, False, N_DST) == (0, 0)                  # the small run
    want = _small_mean(c, name)
    close(want, c.ref[ref_key])
    with env(HGNN_HOT_ROWS=hot, HGNN_HOT_ROWS_H="7"):
        if name in HOT_VARIANTS:
            side = "bwd" if name.startswith("k2") else "fwd"
            rel = c.big[3] if side == "bwd" else c.big[2]
            hc = rel.hot_cols(side, N_SRC * d * (2 if name == "k1_bf16" else 4))
            assert (hc is not None and 0 < hc.share < 1) if hot == "force" else hc is None
        out = _mean_run(c, name, "big")
    assert tuple(out.shape) == (c.n_big, d)
    got = out[c.md]
    print("mean", d, name, hot, float((got.double().cpu() - c.ref[ref_key]).abs().max()))
    close(got, c.ref[ref_key])
    assert torch.equal(got, want), "differs from the small-table run"
    if rest == "zero":
        assert only_mapped_rows_are_written(out, c.md)
    elif rest == "prior":
        assert only_mapped_rows_are_written(out, c.md, PRIOR)
    else:       # unmapped rows below the limit kept the prior (+ 0); the others were written fresh
        lim = int(c.md[ACC_LIMIT])
        out[c.md[:ACC_LIMIT]] = PRIOR
        out[c.md[ACC_LIMIT:]] = 0.0
        assert bool((out[:lim] == PRIOR).all()) and int(torch.count_nonzero(out[lim:])) == 0


MEAN_PARAMS = [(n, None) for n in VARIANTS] + [(n, "force") for n in HOT_VARIANTS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,hot", MEAN_PARAMS,
                         ids=[f"{n}-{'force' if h else 'unset'}" for n, h in MEAN_PARAMS])
def test_mean_gathers_above_the_output_gate(mean_case, name, hot):
    """K1 / K2 writing their rows with ``store_nt`` (the ``accumulate`` read-add-store included),
    plain, weighted, bf16 source rows, ``acc_limit``, and the two-policy loads under
    ``HGNN_HOT_ROWS=force``."""
    _check_mean_variant(mean_case, name, hot)


@pytest.mark.gpu
def test_scalar_shape_mean_gather_above_the_output_gate():
    """d = 20, one float per lane: ``ops.gather_mean`` fresh, 13.4M output rows."""
    _check_mean_variant(build_mean_case(20), "k1_mean", None)
    _release()


@pytest.mark.gpu
def test_two_job_gather_mean_many_above_the_output_gate(mean_case, monkeypatch):
    """``hgnn_gather_reduce_multi``: one job above the gate and one below it in one launch."""
    from truth_recommendation_gnn_amd.graph import NO_SPLIT
    c = mean_case
    b = c.b
    small = relations(b.src, b.dst, N_SRC, N_DST, chunk=NO_SPLIT)
    big = relations(b.src, c.md.cpu()[b.dst], N_SRC, c.n_big, chunk=NO_SPLIT)
    assert small[2].fwd.plan.n_heavy == 0 and big[2].fwd.plan.n_heavy == 0
    calls = []
    real = ops._gather_multi
    monkeypatch.setattr(ops, "_gather_multi",
                        lambda jobs, **kw: (calls.append(len(jobs)), real(jobs, **kw))[1])
    with env(HGNN_HOT_ROWS="0"):
        want = ops.gather_mean_many([(c.x, small[2]), (c.x2, small[2])])
        got = ops.gather_mean_many([(c.x, big[2]), (c.x2, small[2])])
    assert calls == [2, 2]                                   # both went through the one launch
    assert gather_nt(N_SRC, c.d, 4, False, c.n_big) == (0, 1)
    assert gather_nt(N_SRC, c.d, 4, False, N_DST) == (0, 0)
    close(want[0], c.ref["mean"])
    close(want[1], c.ref["mean2"])
    assert torch.equal(got[1], want[1])
    rows = got[0][c.md]
    close(rows, c.ref["mean"])
    assert torch.equal(rows, want[0])
    assert only_mapped_rows_are_written(got[0], c.md)


# ----------------------------------------------------------------------------- GPU: hot rows
@pytest.mark.gpu
@pytest.mark.parametrize("d", (128, 64))
def test_hot_rows_engage_on_their_own(d):
    """K1 and K2 over a 256-MiB source table with ``HGNN_HOT_ROWS`` unset: the policy turns the
    two-policy loads on by itself, and the results are bitwise those under ``HGNN_HOT_ROWS=0``."""
    _release()
    lib = N.lib()
    b = gather_inputs(d)
    with env(HGNN_HOT_ROWS=None):
        n_src = smallest(lambda n: lib.hgnn_hot_rows_policy(n * d * 4, 1, 1.0))
        assert lib.hgnn_hot_rows_policy((n_src - 1) * d * 4, 1, 1.0) == 0
        assert lib.hgnn_hot_rows_policy(N_SRC * d * 4, 1, 1.0) == 0
    assert n_src * d * 4 == 256 * MIB
    ms = torch.from_numpy(idmap(N_SRC, n_src, 400 + d))
    ei, ei_up, k1, k2 = relations(ms[b.src], b.dst, n_src, N_DST)
    assert k1.fwd.plan.n_heavy == 3 and k2.bwd.plan.n_heavy == 3
    x = embed(b.x, ms.to(dev()), n_src)
    pre = b.pre.to(dev())
    nbytes = x.numel() * 4
    assert gather_nt(n_src, d, 4, False, N_DST) == (0, 0)

    def run_all():
        return {"mean": ops.gather_mean(x, k1),
                "k2": ops.scatter_mean_bwd(x, k2),
                "k2+pre": ops.scatter_mean_bwd(x, k2, out=pre.clone()),
                "k2+pre_lim": _raw_k2(k2, x, pre.clone(), ACC_LIMIT, k2.hot_cols("bwd", nbytes))}

    with env(HGNN_HOT_ROWS=None, HGNN_HOT_ROWS_H="13"):
        for rel, side in ((k1, "fwd"), (k2, "bwd")):
            hc = rel.hot_cols(side, nbytes)
            assert hc is not None and hc.h == 13 and 0.5 <= hc.share < 1.0, side
            assert lib.hgnn_hot_rows_policy(nbytes, 1, hc.share) == 1
            assert int((hc.col < 0).sum()) == round(hc.share * hc.col.numel())
        got = run_all()
    with env(HGNN_HOT_ROWS="0", HGNN_HOT_ROWS_H="13"):
        assert k1.hot_cols("fwd", nbytes) is None and k2.hot_cols("bwd", nbytes) is None
        want = run_all()
    for name in got:
        close(want[name], b.ref[name])
        assert torch.equal(got[name], want[name]), name
    del x, got, want, k1, k2, ei, ei_up
    _release()


# ----------------------------------------------------------------------------- GPU: past 2^31
def _rows31():
    """The last 8 rows and 1000 seeded rows of an N31-row table."""
    r = torch.randint(0, N31, (1000,), generator=torch.Generator().manual_seed(31))
    return torch.cat([torch.arange(N31 - 8, N31), r])


TABLE31 = N31 * D31 * 4                    # bytes of one fp32 table of that size


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("fp32", "bf16", "zp"))
def test_loss_with_both_tables_past_2_31_elements(kind):
    """Users and posts embedded into 2^24 + 8 rows at d = 128: the mapped last rows of U, P, dU
    and dP lie past element index 2^31."""
    _release()
    e = elem_of(kind)
    # U and P (e bytes per element), dU and dP (fp32), the packed copy (640 B per row), and the
    # temporaries of the checks (a row gather, a bool per element) with the sort's buffers: 2 GiB
    need = 2 * N31 * D31 * e + 2 * TABLE31 + (N31 * 640 if kind == "zp" else 0) + 2 * GIB
    require_free(need)
    assert (N31 - 8) * D31 >= 2**31
    c = embedded_loss_case(D31, kind, N31, N31)
    assert int(c.mu[-1]) == N31 - 1 and int(c.mp[-2]) == N31 - 2
    assert score_nt(N31, D31, kind == "bf16") == 1 and one_pass(N31) == 0
    assert gather_nt(N31, D31, e, True, N31) == (1, 1)
    with env(HGNN_ZPACK=None):
        assert ops.zpack_on(c.U, bool(getattr(c.U, ops.RELU_OUT, False))) == (kind == "zp")
    check_loss_mode(c, 1, "mean", "2^31")
    _release()


@pytest.mark.gpu
@pytest.mark.parametrize("side", ("source", "destination"))
def test_k1_reads_and_writes_a_row_past_2_31_elements(side):
    _release()
    require_free(TABLE31 + 2 * GIB)                          # the table, a bool per element of it
    d = D31
    b = gather_inputs(d)
    small = relations(b.src, b.dst, N_SRC, N_DST)
    with env(HGNN_HOT_ROWS="0"):
        want = ops.gather_mean(b.x.to(dev()), small[2])
    close(want, b.ref["mean"])
    with env(HGNN_HOT_ROWS=None):
        if side == "source":
            ms = torch.from_numpy(idmap(N_SRC, N31, 31))
            assert int(ms[-1]) * d >= 2**31
            rel = relations(ms[b.src], b.dst, N31, N_DST)
            x = embed(b.x, ms.to(dev()), N31)
            got = ops.gather_mean(x, rel[2])
        else:
            md = torch.from_numpy(idmap(N_DST, N31, 32))
            assert int(md[-1]) * d >= 2**31
            assert gather_nt(N_SRC, d, 4, False, N31) == (0, 1)
            rel = relations(b.src, md[b.dst], N_SRC, N31)
            out = ops.gather_mean(b.x.to(dev()), rel[2])
            got = out[md.to(dev())]
            assert only_mapped_rows_are_written(out, md.to(dev()))
    close(got, b.ref["mean"])
    assert torch.equal(got, want)
    assert float(got[-1].abs().max()) > 0                    # the last row has edges
    _release()


@pytest.fixture(scope="module")
def table31():
    """A dense normal table of 2^24 + 8 rows x 128 and its ReLU."""
    _release()
    require_free(2 * TABLE31 + N31 * 640 + 2 * GIB)          # T, R, the largest output, slack
    T = torch.randn(N31, D31, device=dev(), generator=torch.Generator(dev()).manual_seed(31))
    h = _holder(T=T, R=torch.relu(T), rows=_rows31().to(dev()))
    yield h
    _release()


@pytest.mark.gpu
def test_rows_to_bf16_past_2_31_elements(table31):
    h = table31
    out = ops.rows_to_bf16(h.T)
    assert tuple(out.shape) == (N31, D31)
    assert torch.equal(out[h.rows], h.T[h.rows].to(torch.bfloat16))


@pytest.mark.gpu
def test_relu_grad_bf16_past_2_31_elements(table31):
    h = table31
    out = ops.relu_grad_bf16(h.T, out_act=h.R)
    want = torch.where(h.R[h.rows] > 0, h.T[h.rows], torch.zeros((), device=dev()))
    assert torch.equal(out[h.rows], want.to(torch.bfloat16))
    assert float(out[h.rows].float().abs().max()) > 0


@pytest.mark.gpu
def test_zpack_rows_past_2_31_elements(table31):
    h = table31
    slot = int(N.lib().hgnn_zpack_slot_bytes(D31))
    assert slot == 640
    packed = ops.zpack_rows(h.R).view(N31, slot)[h.rows].cpu().numpy()
    bits = h.R[h.rows].cpu().numpy().view(np.uint32)
    for r in range(bits.shape[0]):
        nz = bits[r] != 0
        vals = bits[r][nz].astype("<u4").view(np.uint8)
        assert np.array_equal(packed[r, :16], np.packbits(nz, bitorder="little")), r
        assert np.array_equal(packed[r, 16:16 + vals.size], vals), r
    assert 0.3 < float((bits == 0).mean()) < 0.7


@pytest.mark.gpu
def test_linear_fwd_past_2_31_elements(table31):
    h = table31
    gen = torch.Generator().manual_seed(131)
    w = (torch.randn(D31, D31, generator=gen) / D31 ** 0.5).to(dev())
    bias = torch.randn(D31, generator=gen).to(dev())
    out = ops.linear_fwd([h.T], w, bias, relu=False)
    assert tuple(out.shape) == (N31, D31)
    ref = h.T[h.rows].double() @ w.double().t() + bias.double()
    close(out[h.rows], ref)
