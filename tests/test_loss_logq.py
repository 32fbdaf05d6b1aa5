"""logQ correction of the link loss: ``logq=`` on ``ops.link_loss``, ``ops.edge_bce_loss`` and
``ops.edge_bce_loss_raw``, ``PostDistribution.log_q`` and the ``_lq`` C entries.

Every scored pair (u, p), positive and negative alike, uses the logit ``<U[u], P[p]> - b[p]``.
The reference is the float64 restatement ``_ref64`` below (``tests/test_neg_sampler.py``'s, with
``- logq[post]`` on both score vectors), cross-checked against ``ops.link_loss(logq=)`` in fp32.
Tolerances are that file's for these kernels on this graph: rtol 1e-4 and atol 1e-5 of the
reference's largest entry; for bf16 rows the reference reads the tables rounded to bf16.

The graph is the one ``tests/test_neg_sampler.py`` builds (rebuilt here): 300 users, 37 posts,
about 3,000 edges, plan chunk 64; one user with 130 edges and one with none; one post heavy in
positives and negatives, one heavy in negatives only (no positives), one heavy in positives only
whose weight is 0 (the clamp of ``log_q``), and light posts.  The negatives are the reference
mapping's draws from that skewed distribution, made on the CPU, so the references need no device
and are shared by every test."""
import ctypes
import functools
import math
import types
from bisect import bisect_right

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N
from truth_recommendation_gnn_amd import ops

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
HGNN_E_ARG, HGNN_E_UNSUPPORTED = 1001, 1004
BCE = torch.nn.functional.binary_cross_entropy_with_logits
DEV = "cuda:0"
N_USERS, N_POSTS = 300, 37
BIG_USER, NO_EDGE_USER = 0, 1
NO_POS, HEAVY = 0, 1                        # posts: no positives / 200 positives
CHUNK = 64
UP = 2.5                                    # the upstream gradient of every backward here
RTOL, ATOL_SCALE = 1e-4, 1e-5
KS = (1, 3)


# ----------------------------------------------------------------------------- reference
def splitmix64(seed: int, c: int) -> int:
    x = (seed + c * GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def ref_draws(seed: int, n: int, cdf):
    tail, T = cdf[1:], cdf[-1]
    return np.array([bisect_right(tail, (splitmix64(seed, c) * T) >> 64) for c in range(n)],
                    dtype=np.int64)


def close(got, ref, rtol=RTOL, atol_scale=ATOL_SCALE):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6)
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol_scale * scale)


def tol(ref):
    """The largest error ``close`` accepts anywhere in ``ref``."""
    m = float(torch.as_tensor(ref).abs().max())
    return RTOL * m + ATOL_SCALE * max(m, 1e-6)


def _graph():
    rng = np.random.default_rng(23)
    deg = rng.integers(40, 121, N_POSTS)
    deg[NO_POS], deg[HEAVY] = 0, 200
    post = np.repeat(np.arange(N_POSTS), deg)
    user = rng.integers(2, N_USERS, post.size)
    big = rng.integers(3, N_POSTS, 130)
    user = np.concatenate([user, np.full(130, BIG_USER)])
    post = np.concatenate([post, big])
    perm = rng.permutation(post.size)
    user, post = user[perm], post[perm]
    assert 2800 <= post.size <= 3400
    return user, post


def _tables(d, relu=False):
    gen = torch.Generator().manual_seed(500 + d)
    U = 0.3 * torch.randn(N_USERS, d, generator=gen)
    P = 0.3 * torch.randn(N_POSTS, d, generator=gen)
    if relu:
        U = torch.relu(U) * 1.5
    return U, P


def _ref64(U, P, ei, neg, w, weighting, logq=None):
    Ur, Pr = U.double().requires_grad_(), P.double().requires_grad_()
    u = Ur[ei[0]]
    sp = (u * Pr[ei[1]]).sum(1)
    sn = (u[:, None, :] * Pr[neg]).sum(-1) if neg.dim() == 2 else (u * Pr[neg]).sum(1)
    if logq is not None:
        b = logq.double()
        sp, sn = sp - b[ei[1]], sn - b[neg]
    neg_loss = BCE(sn, torch.zeros_like(sn))
    if weighting == "edge":
        loss = (w.double() * BCE(sp, torch.ones_like(sp), reduction="none")).mean() + neg_loss
    else:
        loss = (w.double() * BCE(sp, torch.ones_like(sp))).mean() + neg_loss
    (loss * UP).backward()
    return loss.detach(), Ur.grad, Pr.grad


def log_q64(q, T, k):
    """The float64 formula of ``PostDistribution.log_q``: log(k max(q, 1) / T)."""
    return torch.log(torch.from_numpy(np.maximum(q, 1)).double() * float(k) / float(T))


@functools.lru_cache(maxsize=None)
def _data():
    """Everything that needs no device: the edges, the skewed distribution (quantised as
    ``PostDistribution`` does), its draws in COO order per k and the logQ tables."""
    user, post = _graph()
    E = post.size
    deg = np.bincount(post, minlength=N_POSTS)
    udeg = np.bincount(user, minlength=N_USERS)
    assert udeg[BIG_USER] == 130 > CHUNK and udeg[NO_EDGE_USER] == 0
    # 0.9 of the mass on the post with 200 positives, 0.05 on the post without positives, none
    # on one post with more than a chunk of positives, the rest spread thin
    pos_only = int(np.nonzero((deg > CHUNK) & (np.arange(N_POSTS) > HEAVY))[0][0])
    w = np.full(N_POSTS, 0.05 / (N_POSTS - 3))
    w[HEAVY], w[NO_POS], w[pos_only] = 0.9, 0.05, 0.0
    q = np.floor(w / w.max() * float(2**32 - 1)).astype(np.int64)
    cdf = [0]
    for v in q:
        cdf.append(cdf[-1] + int(v))
    T = cdf[-1]
    neg, b = {}, {}
    for k in KS:
        draws = ref_draws(0x1234567890ABCDEF + k, E * k, cdf)
        cnt = np.bincount(draws, minlength=N_POSTS)
        assert deg[HEAVY] > CHUNK and cnt[HEAVY] > CHUNK              # heavy in both
        assert deg[NO_POS] == 0 and cnt[NO_POS] > CHUNK               # heavy negatives only
        assert deg[pos_only] > CHUNK and cnt[pos_only] == 0           # heavy positives only
        assert ((deg <= CHUNK) & (cnt <= CHUNK) & (deg > 0) & (cnt > 0)).any()   # light
        neg[k] = torch.from_numpy(draws.reshape((E,) if k == 1 else (E, k)))    # COO order
        b[k] = log_q64(q, T, k).float()
        assert bool(torch.isfinite(b[k]).all()) and q[pos_only] == 0
    ei = torch.from_numpy(np.stack([user, post]))
    pw = torch.where(torch.arange(E) % 3 == 0, 3.0, 1.0)
    return types.SimpleNamespace(ei=ei, E=E, w=w, q=q, T=T, neg=neg, b=b, pw=pw,
                                 pos_only=pos_only, refs={})


def _ref(U, P, key, k, weighting, logq=True):
    """The float64 reference of one (tables, k, weighting), with or without the table: computed
    once per ``key`` and never changed."""
    D = _data()
    full = (key, k, weighting, logq)
    if full not in D.refs:
        D.refs[full] = _ref64(U, P, D.ei, D.neg[k], D.pw, weighting, D.b[k] if logq else None)
    return D.refs[full]


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("weighting", ("mean", "edge"))
def test_reference_discriminates_and_link_loss_matches_it(k, weighting):
    """On the reference alone: the loss and both gradients with the table differ from those
    without it by more than 100 x the tolerance, so a kernel that ignored the table could not
    pass.  Then ``ops.link_loss(logq=)`` in fp32 against the float64 formula, for [E] and [E, 3]
    negatives and both weightings."""
    D = _data()
    U, P = _tables(64)
    ref = _ref(U, P, (64, "fp32"), k, weighting)
    plain = _ref(U, P, (64, "fp32"), k, weighting, logq=False)
    for a, b, name in zip(ref, plain, ("loss", "dU", "dP")):
        gap = float((a - b).abs().max())
        print(k, weighting, name, "gap", gap, "tolerance", tol(a))
        assert gap > 100 * tol(a), name
    Uf, Pf = U.clone().requires_grad_(), P.clone().requires_grad_()
    loss = ops.link_loss(Uf, Pf, D.ei, D.neg[k], D.pw, weighting=weighting, logq=D.b[k])
    (loss * UP).backward()
    for a, b in zip((loss, Uf.grad, Pf.grad), ref):
        close(a, b)


def test_link_loss_without_logq_is_the_function_it_was():
    D = _data()
    U, P = _tables(16)
    for k in KS:
        neg = D.neg[k]
        for weighting in ("mean", "edge"):
            u = U[D.ei[0]]
            ps = (u * P[D.ei[1]]).sum(dim=1)
            ns = ((u[:, None, :] * P[neg]).sum(dim=-1) if neg.dim() == 2
                  else (u * P[neg]).sum(dim=1))
            nl = BCE(ns, torch.zeros_like(ns))
            if weighting == "edge":
                want = (D.pw * BCE(ps, torch.ones_like(ps), reduction="none")).mean() + nl
            else:
                want = (D.pw * BCE(ps, torch.ones_like(ps))).mean() + nl
            assert torch.equal(ops.link_loss(U, P, D.ei, neg, D.pw, weighting=weighting), want)
            assert torch.equal(ops.link_loss(U, P, D.ei, neg, D.pw, weighting, None), want)


def test_link_loss_gradients_flow_to_the_embeddings_and_not_to_logq():
    D = _data()
    U, P = _tables(16)
    U.requires_grad_()
    P.requires_grad_()
    b = D.b[3].clone().requires_grad_()
    loss = ops.link_loss(U, P, D.ei, D.neg[3], D.pw, logq=b)
    loss.backward()
    assert float(U.grad.abs().max()) > 0 and float(P.grad.abs().max()) > 0
    assert b.grad is None
    # a table in float64 or float16 is cast, not refused
    for dt in (torch.float64, torch.float16):
        close(ops.link_loss(U, P, D.ei, D.neg[3], D.pw, logq=D.b[3].to(dt)), loss,
              rtol=2e-3 if dt == torch.float16 else RTOL)


def test_argument_errors_that_need_no_device():
    ei = torch.tensor([[0, 1, 2], [1, 0, 1]])
    U, P, w, one = torch.randn(3, 8), torch.randn(2, 8), torch.ones(3), torch.ones(())
    neg = torch.tensor([0, 1, 0])
    good = torch.zeros(2)
    calls = {
        "link_loss": lambda **kw: ops.link_loss(U, P, ei, neg, w, **kw),
        "edge_bce_loss": lambda **kw: ops.edge_bce_loss(U, P, ei, neg, w, **kw),
        "edge_bce_loss_raw": lambda **kw: ops.edge_bce_loss_raw(U, P, ei, neg, 3, one, **kw),
    }
    for who, call in calls.items():
        for bad in (torch.zeros(3), torch.zeros(2, 1), torch.zeros(())):
            with pytest.raises(ValueError, match=rf"{who}: logq of shape .* expected \[2\]"):
                call(logq=bad)
        for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.bool), [0., 0.]):
            with pytest.raises(ValueError, match=f"{who}: logq must be a floating tensor"):
                call(logq=bad)
    # the sharded step's arguments: an error, never a fallback to the uncorrected scores
    with pytest.raises(ValueError, match="edge_bce_loss: logq does not combine with ready"):
        calls["edge_bce_loss"](logq=good, ready=lambda: None)
    for kw in ({"ready": lambda: None}, {"on_dP": lambda dP: None}, {"p_chunks": [(0, 2, None)]}):
        with pytest.raises(ValueError, match="edge_bce_loss_raw: logq does not combine with "
                           + next(iter(kw))):
            calls["edge_bce_loss_raw"](logq=good, **kw)
    with pytest.raises(ValueError, match="logq does not combine with ready / on_dP / p_chunks"):
        ops._edge_bce(U, P, None, neg, one, False, 3, ready=lambda: None, logq=good)
    # a table that passes these rules reaches the device check, as every other argument does
    with pytest.raises(ValueError, match="runs only on a ROCm GPU"):
        calls["edge_bce_loss"](logq=good)


def test_c_entries_check_their_arguments_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_int64 * 4)()
    x = ctypes.c_void_p(ctypes.addressof(buf))     # non-null, never dereferenced

    def err():
        return lib.hgnn_last_error_string()

    for name in ("hgnn_edge_score_fwd_k_lq", "hgnn_edge_score_fwd_k_lq_bf16"):
        fn, who = getattr(lib, name), name[len("hgnn_"):].encode()

        def score(d=64, n_posts=9, edge_w=None, i64=None, i32=x, seed=None, n_neg=2, bias=x):
            return fn(x, x, d, 4, n_posts, x, x, edge_w, i64, i32, seed, n_neg, 10, x, bias, x, x,
                      x, None, None)

        assert score(bias=None) == HGNN_E_ARG and who + b": post_bias is null" in err()
        assert score(n_neg=0) == HGNN_E_ARG and who + b": n_neg=0" in err()
        assert score(i64=x) == HGNN_E_ARG and b"exactly one form" in err()
        assert score(i32=None) == HGNN_E_ARG and b"exactly one form" in err()
        assert score(i32=None, seed=x, n_posts=0) == HGNN_E_ARG and b"out of range" in err()
        assert score(d=0) == HGNN_E_ARG and b"bad sizes" in err()
        assert score(d=520) == HGNN_E_UNSUPPORTED and who in err()
    assert lib.hgnn_edge_score_fwd_k_lq_bf16(x, x, 12, 4, 9, x, x, None, None, x, None, 2, 10, x,
                                             x, x, x, x, None, None) == HGNN_E_UNSUPPORTED
    assert b"bf16 rows need" in err()

    def gather(rows=0, d=64, rowptr_n=x, bias=x):
        return lib.hgnn_score_gather2_lq(rows, x, 4, x, d, x, x, None, rowptr_n, x, 4, x, 0.5,
                                         bias, None, None, 0, 0, 64, None, x, None)

    assert gather(rows=3) == HGNN_E_ARG and b"score_gather2_lq: rows=3" in err()
    assert gather(rows=-1) == HGNN_E_ARG and b"rows=-1" in err()
    assert gather(bias=None) == HGNN_E_ARG and b"score_gather2_lq: row_bias is null" in err()
    assert gather(rowptr_n=None) == HGNN_E_ARG and b"rowptr_n is null" in err()
    assert gather(d=0) == HGNN_E_ARG and b"bad sizes" in err()
    assert gather(rows=1, d=12) == HGNN_E_UNSUPPORTED and b"bf16 rows need" in err()
    assert gather(rows=2, d=32) == HGNN_E_UNSUPPORTED and b"zero-packed" in err()

    def planned(rows=0, d=64, rowptr_n=x, counts=x, out=x, bias=x):
        return lib.hgnn_score_gather2_planned_lq(rows, x, 4, x, d, x, x, None, rowptr_n, x, 4, x,
                                                 0.5, bias, None, None, 0, 0, 64, None, x, x,
                                                 counts, 8, x, out, None)

    assert planned(rows=3) == HGNN_E_ARG and b"score_gather2_planned_lq: rows=3" in err()
    assert planned(bias=None) == HGNN_E_ARG and b"planned_lq: row_bias is null" in err()
    assert planned(d=0) == HGNN_E_ARG and b"bad sizes" in err()
    assert planned(rowptr_n=None) == HGNN_E_ARG and b"null rowptr" in err()
    assert planned(out=None) == HGNN_E_ARG
    assert planned(counts=None) == HGNN_E_ARG and b"null arrays" in err()
    assert planned(rows=1, d=12) == HGNN_E_UNSUPPORTED and b"bf16 rows need" in err()
    assert planned(rows=2, d=32) == HGNN_E_UNSUPPORTED and b"zero-packed" in err()


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def g():
    D = _data()
    dev = torch.device(DEV)
    ei_d = D.ei.to(dev)
    csr = ops.relation_csr_for_loss(ei_d, N_USERS, N_POSTS)
    assert csr.fwd.plan.chunk == CHUNK and csr.fwd.plan.n_heavy > 0
    perm_u = csr.bwd.perm.cpu().long()       # user-grouped position -> COO edge
    dist = ops.PostDistribution(torch.from_numpy(D.w).to(dev))
    assert np.array_equal(dist.q.cpu().numpy(), D.q) and dist.T == D.T
    sk, b = {}, {}
    for k in KS:
        sk[k] = ops.SkewedNegatives(D.neg[k][perm_u].to(torch.int32).contiguous().to(dev))
        b[k] = dist.log_q(k)
    return types.SimpleNamespace(dev=dev, ei_d=ei_d, csr=csr, E=D.E, sk=sk, b=b, dist=dist,
                                 perm_u=perm_u, pos_only=D.pos_only, D=D)


_IN = {}


def _inputs(g, d, rows):
    """Tables and weights of one width and row format: built once."""
    key = (d, rows)
    if key not in _IN:
        U, P = _tables(d, relu=rows == "zp")
        Ud, Pd = U.to(g.dev), P.to(g.dev)
        if rows == "bf16":      # the reference reads the numbers the kernels read
            U, P = ops.rows_to_bf16(Ud).float().cpu(), ops.rows_to_bf16(Pd).float().cpu()
        _IN[key] = types.SimpleNamespace(U=U, P=P, Ud=Ud, Pd=Pd, wd=g.D.pw.to(g.dev), key=key)
    return _IN[key]


def _run(g, t, neg, rows, logq, neg_order="user", **kw):
    U, P = t.Ud.clone().requires_grad_(), t.Pd.clone().requires_grad_()
    extra = {} if logq is None else {"logq": logq}
    loss = ops.edge_bce_loss(U, P, g.ei_d, neg, t.wd, neg_order=neg_order,
                             row_dtype="bf16" if rows == "bf16" else "fp32", **extra, **kw)
    (loss * UP).backward()
    return loss.detach(), U.grad, P.grad


def _timed_names(fn):
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        res = fn()
    finally:
        ops.set_timer(None)
    return res, [r[0] for r in timer.records]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_log_q_is_the_float64_formula_cast(g, k):
    got = g.dist.log_q(k)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N_POSTS,) and got.device == g.dev
    assert bool(torch.isfinite(got).all())
    want = log_q64(g.dist.q.cpu().numpy(), g.dist.T, k)
    err = (got.double().cpu() - want).abs()
    print("log_q", k, float(err.max()), float(want.abs().max()))
    assert bool((err <= 2.0 ** -23 * want.abs()).all())      # fp32 rounding, one ulp at the most
    # the post of weight 0 gets the smallest drawable weight's offset; a heavier post a larger one
    low = math.log(k / g.dist.T)
    assert abs(float(got[g.pos_only]) - low) <= 2.0 ** -23 * abs(low)
    assert float(got[HEAVY]) > float(got[NO_POS]) > float(got[g.pos_only])
    assert g.dist.log_q(k) is got                             # one tensor per k: checked once
    with pytest.raises(ValueError, match="num_neg"):
        g.dist.log_q(0)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ("fp32", "bf16", "zp"))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", (64, 128))
def test_fused_loss_with_logq_matches_float64(g, d, k, rows, monkeypatch):
    monkeypatch.setenv("HGNN_ZPACK", "1" if rows == "zp" else "0")
    t = _inputs(g, d, rows)
    sk = g.sk[k]
    for weighting in ("mean", "edge"):
        ref = _ref(t.U, t.P, t.key, k, weighting)
        got, names = _timed_names(lambda: _run(g, t, sk, rows, g.b[k], weighting=weighting))
        assert f"score_gather_planned[{N_POSTS}<-{N_USERS}]x{d}" in names
        assert "plan_negatives" in names and f"edge_score_d{d}" in names
        assert (f"zpack[{N_USERS}]x{d}" in names) == (rows == "zp")
        for a, b, name in zip(got, ref, ("loss", "dU", "dP")):
            print(d, k, rows, weighting, name, float((a.double().cpu() - b).abs().max()),
                  float(b.abs().max()))
            close(a, b)
        for p in (HEAVY, NO_POS, g.pos_only):
            assert float(got[2][p].abs().max()) > 0
        assert float(got[1][NO_EDGE_USER].abs().max()) == 0
        again = _run(g, t, sk, rows, g.b[k], weighting=weighting)
        for a, b, name in zip(again, got, ("loss", "dU", "dP")):
            assert torch.equal(a, b), name
        # the same negatives as a plain tensor: the unplanned gather, the same numbers
        plain, names = _timed_names(lambda: _run(g, t, sk.values, rows, g.b[k],
                                                 weighting=weighting))
        assert f"score_gather[{N_POSTS}<-{N_USERS}]x{d}" in names
        assert "plan_negatives" not in names
        for a, b in zip(plain, ref):
            close(a, b)
        for a, b in zip(plain, got):
            close(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", (5, 200))
def test_odd_widths(g, d, k):
    """d = 5 (scalar rows) and d = 200 (two vectors per lane), fp32."""
    t = _inputs(g, d, "fp32")
    ref = _ref(t.U, t.P, t.key, k, "edge")
    for neg in (g.sk[k], g.sk[k].values):
        got = _run(g, t, neg, "fp32", g.b[k], weighting="edge")
        for a, b in zip(got, ref):
            close(a, b)


@pytest.mark.gpu
def test_int64_negatives_in_coo_order_and_a_negative_draw(g):
    t = _inputs(g, 64, "fp32")
    got = _run(g, t, g.D.neg[1].to(g.dev), "fp32", g.b[1], neg_order="edge")
    for a, b in zip(got, _ref(t.U, t.P, t.key, 1, "mean")):
        close(a, b)
    draw = ops.draw_negatives(g.ei_d, N_POSTS, torch.Generator(g.dev).manual_seed(9), num_neg=3)
    assert isinstance(draw, ops.NegativeDraw) and tuple(draw.shape) == (g.E, 3)
    neg_edge = torch.empty(g.E, 3, dtype=torch.int64)
    neg_edge[g.perm_u] = draw.tensor().cpu().long()
    ref = _ref64(t.U, t.P, g.D.ei, neg_edge, g.D.pw, "edge", g.D.b[3])
    got = _run(g, t, draw, "fp32", g.b[3], weighting="edge")
    for a, b in zip(got, ref):
        close(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_retained_graph_presorted_and_raw(g, k):
    t = _inputs(g, 64, "fp32")
    sk, b = g.sk[k], g.b[k]
    U, P = t.Ud.clone().requires_grad_(), t.Pd.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, sk, t.wd, neg_order="user", row_dtype="fp32",
                             weighting="edge", logq=b)
    first = torch.autograd.grad(loss, (U, P), retain_graph=True)
    second = torch.autograd.grad(loss, (U, P), retain_graph=True)
    for a, c, name in zip(second, first, ("dU", "dP")):
        assert torch.equal(a, c), name
    close(first[1] * UP, _ref(t.U, t.P, t.key, k, "edge")[2])
    # a presort does not depend on the table: the direct call's numbers, bitwise
    pre = ops.presort_negatives(N_USERS, N_POSTS, g.ei_d, sk, "user")
    want = _run(g, t, sk, "fp32", b, weighting="edge")
    got = _run(g, t, sk, "fp32", b, weighting="edge", presorted=pre)
    for a, c, name in zip(got, want, ("loss", "dU", "dP")):
        assert torch.equal(a, c), name
    # edge_bce_loss_raw: the forward and the unit-gradient backward of edge_bce_loss
    U, P = t.Ud.clone().requires_grad_(), t.Pd.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, sk, t.wd, neg_order="user", row_dtype="fp32", logq=b)
    dU, dP = torch.autograd.grad(loss, (U, P))
    raw = ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, sk, g.E, t.wd.mean(), neg_order="user",
                                logq=b)
    for a, c, name in zip(raw, (loss.detach(), dU, dP), ("loss", "dU", "dP")):
        assert torch.equal(a, c), name
    close(raw[0], _ref(t.U, t.P, t.key, k, "mean")[0])
    raw_pre = ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, sk, g.E, t.wd.mean(), neg_order="user",
                                    presorted=pre, logq=b)
    for a, c in zip(raw_pre, raw):
        assert torch.equal(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_a_zero_table_and_the_default_path(g, k, monkeypatch):
    monkeypatch.setenv("HGNN_ZPACK", "0")
    t = _inputs(g, 64, "fp32")
    zero = torch.zeros(N_POSTS, device=g.dev)
    for neg in (g.sk[k], g.sk[k].values):
        without, names = _timed_names(lambda: _run(g, t, neg, "fp32", None, weighting="edge"))
        # the timer names of the call without logq, as on the parent commit
        planned = ["sort_negatives", "plan_negatives",
                   f"score_gather_planned[{N_POSTS}<-{N_USERS}]x64", "edge_score_d64"]
        unplanned = ["sort_negatives", f"score_gather[{N_POSTS}<-{N_USERS}]x64", "edge_score_d64"]
        assert names == (planned if neg is g.sk[k] else unplanned)
        ref = _ref(t.U, t.P, t.key, k, "edge", logq=False)
        got = _run(g, t, neg, "fp32", zero, weighting="edge")
        for a, c, r in zip(got, without, ref):
            close(c, r)
            close(a, r)
            close(a, c)


@pytest.mark.gpu
def test_errors_that_need_the_device(g):
    t = _inputs(g, 64, "fp32")
    for bad in (float("nan"), float("inf"), float("-inf")):
        b = g.b[1].clone()
        b[g.pos_only] = bad
        with pytest.raises(ValueError, match="logq must be finite"):
            _run(g, t, g.sk[1], "fp32", b)
    # checked once per tensor object and version: an in-place change is seen
    b = g.b[1].clone()
    _run(g, t, g.sk[1], "fp32", b)
    assert ops.logq_table(g.csr, b) is ops.logq_table(g.csr, b)
    b[3] = float("nan")
    with pytest.raises(ValueError, match="logq must be finite"):
        _run(g, t, g.sk[1], "fp32", b)
    with pytest.raises(ValueError, match="runs only on a ROCm GPU"):
        _run(g, t, g.sk[1], "fp32", g.b[1].cpu())
    # a float64 table is cast; an out-of-range int64 negative still raises with check=True
    got = _run(g, t, g.sk[1], "fp32", g.b[1].double())
    for a, c in zip(got, _run(g, t, g.sk[1], "fp32", g.b[1])):
        assert torch.equal(a, c)
    neg = g.D.neg[1].clone()
    neg[5] = N_POSTS + 3
    with pytest.raises(ValueError, match="negative post id out of range"):
        _run(g, t, neg.to(g.dev), "fp32", g.b[1], neg_order="edge", check=True)
