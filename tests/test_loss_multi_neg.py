"""k negatives per positive edge in the fused link loss (``neg_p`` of shape ``[E, k]``).

    loss = <positive term> + 1/(E k) sum_e sum_j softplus(<U[u_e], P[n_e,j]>)

against float64 autograd of that expression written out here, for each weighting of the positive
term, every row format the two loss kernels read (fp32, bf16, zero-packed fp32) and every form of
negatives (int64 in edge order, int32 in user order, a ``NegativeDraw``).

Graph and tables: those of ``tests/test_loss_edge_weights.py`` (``_graph``, ``_tables``, copied).
300 users, 37 posts, about 3000 shuffled positives; one user with 130 positives (three 64-edge
chunks of the scoring pass, the last partial) and one with none; one post with 200 positives (the
heavy-row slab of the dP gather) and one without positives.

Negatives: ``[E, k]`` for k in (2, 3, 5): 3 is no power of two (a sweep of two columns and none
left, after the first), 5 exceeds the edges per step of the d = 128 kernels; 2 leaves a last sweep
of one column.  Post ``NO_NEG`` is remapped away in every column; post ``ONLY_LAST`` has no
positives and is remapped out of every column but k - 1, where it is placed, so a non-zero
``dP[ONLY_LAST]`` shows that the last column is read.  (For a ``NegativeDraw`` the columns are
what the seed gives: the float64 reference takes the same draws, and that row check is skipped.)

Tolerance: the project's fp32 bar against float64, ``close`` of ``tests/test_gpu_parity.py``
(rtol 1e-4, atol 1e-5 of the reference's largest entry)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N
from truth_recommendation_gnn_amd import ops

N_USERS, N_POSTS = 300, 37
BIG_USER, NO_EDGE_USER = 0, 1
NO_POS, HEAVY, NO_NEG = 0, 1, 2            # posts
ONLY_LAST = NO_POS                         # without positives; a negative in column k - 1 only
KS = (2, 3, 5)
DS = (64, 128, 5, 200, 16, 8)
DS_BF16 = tuple(d for d in DS if d % 8 == 0)
DS_ZP = (64, 128)
FORMS = ("i64_edge", "i32_user", "draw")
UP = 2.5                                   # the upstream gradient
RTOL, ATOL_SCALE = 1e-4, 1e-5
HGNN_E_ARG, HGNN_E_UNSUPPORTED = 1001, 1004
BCE = torch.nn.functional.binary_cross_entropy_with_logits


def close(got, ref, rtol=RTOL, atol_scale=ATOL_SCALE):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6)
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol_scale * scale)


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
    assert not (neg == NO_NEG).any() and not (neg[:, :k - 1] == ONLY_LAST).any()
    assert (neg[:, k - 1] == ONLY_LAST).sum() >= E // 7
    return torch.from_numpy(neg)


def _scores64(U, P, ei):
    return (U.double()[ei[0]] * P.double()[ei[1]]).sum(1)


def _weights(U, P, ei):
    s = _scores64(U, P, ei)
    return torch.where(s < s.median(), 3.0, 1.0).float()


def _ref64(U, P, ei, neg, w, weighting):
    """float64 autograd of the loss written out: (loss, dU, dP) for the upstream gradient UP."""
    Ur, Pr = U.double().requires_grad_(), P.double().requires_grad_()
    u = Ur[ei[0]]
    sp = (u * Pr[ei[1]]).sum(1)
    sn = (u[:, None, :] * Pr[neg]).sum(-1) if neg.dim() == 2 else (u * Pr[neg]).sum(1)
    neg_loss = BCE(sn, torch.zeros_like(sn))               # the mean over all E k
    if weighting == "edge":
        loss = (w.double() * BCE(sp, torch.ones_like(sp), reduction="none")).mean() + neg_loss
    else:
        loss = (w.double() * BCE(sp, torch.ones_like(sp))).mean() + neg_loss
    (loss * UP).backward()
    return loss.detach(), Ur.grad, Pr.grad


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", KS)
def test_link_loss_is_the_per_edge_per_negative_sum(k):
    user, post, neg1 = _graph()
    ei, neg1 = torch.from_numpy(np.stack([user, post])), torch.from_numpy(neg1)
    E = ei.shape[1]
    neg = _negatives(E, k)
    U, P = (t.double() for t in _tables(8))
    w = _weights(U, P, ei).double()
    sp = _scores64(U, P, ei)
    sn = torch.stack([_scores64(U, P, torch.stack([ei[0], neg[:, j]])) for j in range(k)], 1)
    for weighting in ("mean", "edge"):
        got = ops.link_loss(U, P, ei, neg, w, weighting=weighting)
        pos, negs = 0.0, 0.0
        for e in range(E):                                 # the explicit loop
            pos += (float(w[e]) if weighting == "edge" else 1.0) * \
                float(np.logaddexp(0.0, -float(sp[e])))
            for j in range(k):
                negs += float(np.logaddexp(0.0, float(sn[e, j])))
        if weighting == "mean":
            pos *= float(w.mean())
        want = pos / E + negs / (E * k)
        assert abs(float(got) - want) <= 1e-12 * abs(want), weighting
    # one negative: the arithmetic of the 1-D form, whichever way it is given
    one = ops.link_loss(U, P, ei, neg1, w)
    u = U[ei[0]]
    today = (w * BCE((u * P[ei[1]]).sum(1), torch.ones(E, dtype=U.dtype))).mean() + \
        BCE((u * P[neg1]).sum(1), torch.zeros(E, dtype=U.dtype))
    assert torch.equal(one, today)
    assert torch.equal(ops.link_loss(U, P, ei, neg1.reshape(E, 1), w), one)
    assert torch.equal(ops.link_loss(U, P, ei, neg1.reshape(E, 1), w, weighting="edge"),
                       ops.link_loss(U, P, ei, neg1, w, weighting="edge"))


def test_argument_errors_that_need_no_device():
    user, post, _ = _graph()
    ei = torch.from_numpy(np.stack([user, post]))
    E = ei.shape[1]
    U, P = _tables(8)
    w, one = torch.ones(E), torch.ones(())
    neg = _negatives(E, 3)
    # a negatives count that is no multiple of E, and shapes that are not [E] / [E, k]
    for bad in (neg.reshape(-1)[:-1], neg.reshape(-1), neg[:-1], neg.t().contiguous()):
        with pytest.raises(ValueError, match=rf"expected \[{E}\].* or \[{E}, k\]"):
            ops.edge_bce_loss(U, P, ei, bad, w)
        with pytest.raises(ValueError, match=rf"expected \[{E}\].* or \[{E}, k\]"):
            ops.edge_bce_loss_raw(U, P, ei, bad, E, one)
        with pytest.raises(ValueError, match=rf"expected \[{E}\].* or \[{E}, k\]"):
            ops.presort_negatives(N_USERS, N_POSTS, ei, bad, "edge")
    # k >= 2 with the sharded step's callbacks
    with pytest.raises(ValueError, match="3 negatives per positive edge do not combine with ready"):
        ops.edge_bce_loss(U, P, ei, neg, w, ready=lambda: None)
    for kw in ({"ready": lambda: None}, {"on_dP": lambda dP: None},
               {"p_chunks": [(0, N_POSTS, None)]}):
        with pytest.raises(ValueError, match="do not combine with " + next(iter(kw))):
            ops.edge_bce_loss_raw(U, P, ei, neg, E, one, **kw)
    # a NegativeDraw of another k, of another E
    seed = torch.zeros(1, dtype=torch.int64)
    draw = ops.NegativeDraw(seed, 3 * E, N_POSTS, 3)
    assert draw.shape == (E, 3) and draw.num_neg == 3 and draw.n == 3 * E
    assert ops.NegativeDraw(seed, E, N_POSTS).shape == (E,)
    assert ops._Negatives.of(draw, E, N_POSTS).k == 3
    with pytest.raises(ValueError, match="NegativeDraw does not match the positive edges"):
        ops.edge_bce_loss(U, P, ei, ops.NegativeDraw(seed, 2 * (E - 1), N_POSTS, 2), w,
                          neg_order="user")
    with pytest.raises(ValueError, match="NegativeDraw does not match the positive edges"):
        ops._Negatives.of(ops.NegativeDraw(seed, 3 * E, N_POSTS, 1), E, N_POSTS)
    with pytest.raises(ValueError, match="no multiple of num_neg"):
        ops.NegativeDraw(seed, 3 * E + 1, N_POSTS, 3)
    pre = ops.PresortedNegatives(None, neg, "edge", N_POSTS, None, None, 3)
    with pytest.raises(ValueError, match="hold 3 per positive edge, the loss got 2"):
        pre.check_draws(_negatives(E, 2), "edge", "edge_bce_loss")
    with pytest.raises(ValueError, match="hold 3 per positive edge, the loss got 2"):
        pre.check_edges(None, N_POSTS, 2)
    # num_neg = 0, and the sort's limit
    for fn in (ops.sample_negatives, ops.draw_negatives):
        with pytest.raises(ValueError, match="num_neg=0"):
            fn(ei, N_POSTS, num_neg=0)
    with pytest.raises(ValueError, match="limit of 2\\^31 - 1"):
        ops._neg_count(ops.NegativeDraw(seed, 2**31, N_POSTS, 4), 2**29, "edge_bce_loss")


def test_new_entries_check_their_arguments_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_int64 * 4)()
    x = ctypes.c_void_p(ctypes.addressof(buf))     # non-null, never dereferenced: the checks
    #                                                below all fail before a launch
    for name, bad_d in (("hgnn_edge_score_fwd_k", 513), ("hgnn_edge_score_fwd_k_bf16", 12)):
        fn = getattr(lib, name)

        def call(d, n_neg, negs=(x, None, None), edge_w=None, n_posts=9):
            return fn(x, x, d, 4, n_posts, x, x, edge_w, *negs, n_neg, 10, x, x, x, x, None, None)

        for w in (None, x):
            assert call(64, 0, edge_w=w) == HGNN_E_ARG
            assert b"n_neg=0" in lib.hgnn_last_error_string()
            assert name[5:].encode() + b":" in lib.hgnn_last_error_string()
        assert call(64, -2) == HGNN_E_ARG
        assert call(64, 3, (x, x, None)) == HGNN_E_ARG
        assert b"exactly one form" in lib.hgnn_last_error_string()
        assert name[5:].encode() + b":" in lib.hgnn_last_error_string()
        assert call(64, 3, (None, None, None)) == HGNN_E_ARG
        assert b"exactly one form" in lib.hgnn_last_error_string()
        assert call(bad_d, 3) == HGNN_E_UNSUPPORTED
        assert b"d=%d" % bad_d in lib.hgnn_last_error_string()
        assert name[5:].encode() + b":" in lib.hgnn_last_error_string()
        assert call(64, 3, (None, None, x), n_posts=0) == HGNN_E_ARG
        assert b"n_posts=0 out of range" in lib.hgnn_last_error_string()
        assert name[5:].encode() + b":" in lib.hgnn_last_error_string()


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def g():
    user, post, neg1 = _graph()
    dev = torch.device("cuda:0")
    ei = torch.from_numpy(np.stack([user, post]))
    ei_d = ei.to(dev)
    E = int(ei.shape[1])
    csr = ops.relation_csr_for_loss(ei_d, N_USERS, N_POSTS)
    assert csr.fwd.plan.n_heavy > 0                         # the 200-edge post is split
    perm_u, perm_p = csr.bwd.perm.cpu().long(), csr.fwd.perm.cpu().long()
    ident = torch.arange(E)
    assert not torch.equal(perm_u, ident) and not torch.equal(perm_p, ident)
    rp_u = csr.bwd.rowptr.cpu()
    assert int(rp_u[BIG_USER + 1] - rp_u[BIG_USER]) == 130
    assert int(rp_u[NO_EDGE_USER + 1] - rp_u[NO_EDGE_USER]) == 0
    # per k the three forms: (what the loss gets, neg_order, the same negatives in edge order)
    forms = {}
    for k in KS:
        neg = _negatives(E, k)
        draw = ops.draw_negatives(ei_d, N_POSTS, num_neg=k,
                                  generator=torch.Generator(dev).manual_seed(7 + k))
        assert draw.shape == (E, k) and draw.n == E * k and draw.num_neg == k
        neg_draw = torch.empty(E, k, dtype=torch.int64)
        neg_draw[perm_u] = draw.tensor().cpu().long()       # back to edge order, for the reference
        forms[k] = {"i64_edge": (neg.to(dev), "edge", neg),
                    "i32_user": (neg[perm_u].to(torch.int32).to(dev), "user", neg),
                    "draw": (draw, "user", neg_draw)}
    return types.SimpleNamespace(dev=dev, ei=ei, ei_d=ei_d, csr=csr, E=E, forms=forms,
                                 neg1=torch.from_numpy(neg1), perm_u=perm_u)


_IN = {}


def _inputs(g, d, relu=False):
    """Tables, weights and the float64 references of one width: built once, never written."""
    key = (d, relu)
    if key not in _IN:
        U, P = _tables(d, relu)
        w = _weights(U, P, g.ei)
        _IN[key] = types.SimpleNamespace(U=U, P=P, w=w, Ud=U.to(g.dev), Pd=P.to(g.dev),
                                         wd=w.to(g.dev), ref={})
    return _IN[key]


def _ref(g, t, k, form, weighting):
    key = (k, form, weighting)
    if key not in t.ref:
        t.ref[key] = _ref64(t.U, t.P, g.ei, g.forms[k][form][2], t.w, weighting)
    return t.ref[key]


def _run(g, U, P, w, neg, order, **kw):
    """edge_bce_loss + backward with the upstream gradient UP: (loss, dU, dP)."""
    U, P = U.clone().requires_grad_(), P.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, neg, w, neg_order=order, **kw)
    (loss * UP).backward()
    return loss.detach(), U.grad, P.grad


def _timed_names(fn):
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        res = fn()
    finally:
        ops.set_timer(None)
    return res, timer.records


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
def test_loss_and_gradients_match_float64(g, d, k):
    t = _inputs(g, d)
    for form in FORMS:
        neg, order, _ = g.forms[k][form]
        for weighting in ("mean", "edge"):
            ref = _ref(g, t, k, form, weighting)
            got = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting=weighting)
            for a, b, name in zip(got, ref, ("loss", "dU", "dP")):
                print(d, k, form, weighting, name, float((a.double().cpu() - b).abs().max()),
                      float(b.abs().max()))
                close(a, b)
            if form != "draw":
                assert float(got[2][ONLY_LAST].abs().max()) > 0     # column k - 1 is read
            assert float(got[1][NO_EDGE_USER].abs().max()) == 0
            assert float(got[2][HEAVY].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_two_runs_and_the_retained_graph_are_bitwise(g, k):
    d = 64
    t = _inputs(g, d)
    for form in FORMS:
        neg, order, _ = g.forms[k][form]
        first = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting="edge")
        again = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting="edge")
        for a, b, name in zip(again, first, ("loss", "dU", "dP")):
            assert torch.equal(a, b), (form, name)
    neg, order, _ = g.forms[k]["i64_edge"]
    U, P = t.Ud.clone().requires_grad_(), t.Pd.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, neg, t.wd, neg_order=order)
    (loss * UP).backward(retain_graph=True)
    g1 = (U.grad.clone(), P.grad.clone())
    U.grad = P.grad = None
    (loss * UP).backward()
    assert torch.equal(U.grad, g1[0]) and torch.equal(P.grad, g1[1])
    close(g1[0], _ref(g, t, k, "i64_edge", "mean")[1])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS_BF16)
def test_bf16_rows(g, d, k):
    t = _inputs(g, d)
    Ur, Pr = ops.rows_to_bf16(t.Ud).float(), ops.rows_to_bf16(t.Pd).float()
    for form in FORMS:
        neg, order, _ = g.forms[k][form]
        for weighting in ("mean", "edge"):
            want = _run(g, Ur, Pr, t.wd, neg, order, weighting=weighting, row_dtype="fp32")
            got = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting=weighting, row_dtype="bf16")
            for a, b in zip(got, want):
                close(a, b)
    again = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting="edge", row_dtype="bf16")
    for a, b, name in zip(again, got, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS_ZP)
def test_zero_packed_rows_are_bitwise_the_unpacked_rows(g, d, k, monkeypatch):
    t = _inputs(g, d, relu=True)
    assert 0.3 < float((t.U == 0).float().mean()) < 0.7
    neg, order, neg_ref = g.forms[k]["i64_edge"]

    def run():
        return ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, neg, g.E, t.wd.mean(), neg_order=order)

    monkeypatch.setenv("HGNN_ZPACK", "0")
    want, rec0 = _timed_names(run)
    monkeypatch.setenv("HGNN_ZPACK", "1")
    got, rec1 = _timed_names(run)
    names0, names1 = [r[0] for r in rec0], [r[0] for r in rec1]
    assert not any(n.startswith("zpack[") for n in names0)
    assert f"zpack[{N_USERS}]x{d}" in names1                    # the pack pass ran
    for n in (f"score_gather[{N_POSTS}<-{N_USERS}]x{d}", f"edge_score_d{d}", "sort_negatives"):
        assert n in names0 and n in names1                      # the entries keep their names
    for a, b, name in zip(got, want, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name
    ref = _ref64(t.U, t.P, g.ei, neg_ref, t.w, "mean")          # and both are the k-negative loss
    close(got[0], ref[0])
    close(got[1] * UP, ref[1])
    close(got[2] * UP, ref[2])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_presorted_negatives(g, k):
    d = 64
    t = _inputs(g, d)
    for form in FORMS:
        neg, order, _ = g.forms[k][form]
        pre = ops.presort_negatives(N_USERS, N_POSTS, g.ei_d, neg, order)
        assert pre.k == k and int(pre.users.numel()) == k * g.E
        assert int(pre.rowptr[-1]) == k * g.E
        want = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting="edge")
        got = _run(g, t.Ud, t.Pd, t.wd, neg, order, weighting="edge", presorted=pre)
        for a, b, name in zip(got, want, ("loss", "dU", "dP")):
            assert torch.equal(a, b), (form, name)
    # a presort made for another k is refused, by either entry point
    other = KS[(KS.index(k) + 1) % len(KS)]
    neg_o, order_o, _ = g.forms[other]["i64_edge"]
    pre = ops.presort_negatives(N_USERS, N_POSTS, g.ei_d, g.forms[k]["i64_edge"][0], order_o)
    with pytest.raises(ValueError, match=f"hold {k} per positive edge, the loss got {other}"):
        ops.edge_bce_loss(t.Ud, t.Pd, g.ei_d, neg_o, t.wd, neg_order=order_o, presorted=pre)
    with pytest.raises(ValueError, match=f"hold {k} per positive edge, the loss got 1"):
        ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, g.neg1.to(g.dev), g.E, t.wd.mean(),
                              neg_order="edge", presorted=pre)


@pytest.mark.gpu
@pytest.mark.parametrize("d", (64, 128, 5, 8))
def test_k_entry_with_one_negative_agrees_with_the_one_negative_entries(g, d):
    """hgnn_edge_score_fwd_k at n_neg = 1 against hgnn_edge_score_fwd_w and hgnn_edge_score_fwd:
    the same operations in the same order (asserted within ``close``; DESIGN says what was seen
    bit for bit)."""
    t = _inputs(g, d)
    lib, ub = N.lib(), g.csr.bwd
    neg_u = g.neg1[g.perm_u].to(g.dev).contiguous()                 # int64, user-grouped order
    ew = ops.edge_weights_in_kernel_order(g.csr, t.wd)
    c = torch.full((), 1.75, device=g.dev)

    def outs():
        return (torch.empty(N_USERS, d, device=g.dev),
                torch.empty(int(lib.hgnn_edge_score_parts(N_USERS)), device=g.dev),
                torch.empty((), device=g.dev))

    head = (N.ptr(t.Ud), N.ptr(t.Pd), d, N_USERS, N_POSTS, N.ptr(ub.rowptr), N.ptr(ub.col))
    s = N.stream_ptr(g.dev)
    for w in (ew.by_user, None):
        dU_k, part_k, loss_k = outs()
        N.check(lib.hgnn_edge_score_fwd_k(*head, N.ptr(w), N.ptr(neg_u), None, None, 1, g.E,
                                          N.ptr(c), N.ptr(dU_k), N.ptr(part_k), N.ptr(loss_k),
                                          None, s), "hgnn_edge_score_fwd_k")
        dU_1, part_1, loss_1 = outs()
        if w is not None:
            N.check(lib.hgnn_edge_score_fwd_w(*head, N.ptr(w), N.ptr(neg_u), None, None, g.E,
                                              N.ptr(c), N.ptr(dU_1), N.ptr(part_1),
                                              N.ptr(loss_1), None, s), "hgnn_edge_score_fwd_w")
        else:
            N.check(lib.hgnn_edge_score_fwd(*head, N.ptr(neg_u), None, g.E, N.ptr(c),
                                            N.ptr(dU_1), None, None, None, None, N.ptr(part_1),
                                            N.ptr(loss_1), None, s), "hgnn_edge_score_fwd")
        print(d, "edge_w" if w is not None else "collapsed", "bitwise:",
              torch.equal(dU_k, dU_1), torch.equal(loss_k, loss_1))
        close(dU_k, dU_1)
        close(loss_k, loss_1)
        assert float(dU_1.abs().max()) > 0


@pytest.mark.gpu
def test_timer_counts_the_rows_and_ids_of_k_negatives(g):
    d, k = 64, 3
    t = _inputs(g, d)
    neg, order, _ = g.forms[k]["i64_edge"]
    recs = []
    for n in (g.neg1.to(g.dev), neg):
        _, r = _timed_names(lambda: ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, n, g.E,
                                                          t.wd.mean(), neg_order=order))
        recs.append({x[0]: x for x in r})
    row_bytes = 4 * d
    grow = recs[1]["edge_score_d64"][1] - recs[0]["edge_score_d64"][1]
    assert grow == 2 * g.E * (row_bytes + 8)
    # the int64 sort: 4 B x (2 + 1 + 4) + 4 B per pair, on 3 E pairs against E
    per_pair = 4 * (2 + 1 + 4) + 4
    assert recs[0]["sort_negatives"][1] == per_pair * g.E
    assert recs[1]["sort_negatives"][1] == per_pair * 3 * g.E


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_out_of_range_id_in_the_last_column(g, k):
    d = 64
    t = _inputs(g, d)
    neg, order, _ = g.forms[k]["i32_user"]
    bad = neg.clone()
    bad[g.E // 2, k - 1] = N_POSTS          # (the key the int64 sort files its invalid ids under)
    with pytest.raises(ValueError, match="negative post id out of range"):
        ops.edge_bce_loss(t.Ud, t.Pd, g.ei_d, bad, t.wd, neg_order=order, check=True)
    # int64 too (counted by the sort's validation pass as well)
    neg, order, _ = g.forms[k]["i64_edge"]
    bad = neg.clone()
    bad[g.E - 1, k - 1] = N_POSTS + 5
    with pytest.raises(ValueError, match="negative post id out of range"):
        ops.edge_bce_loss(t.Ud, t.Pd, g.ei_d, bad, t.wd, neg_order=order, check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("d", (64, 5))
def test_one_column_is_the_one_negative_path(g, d):
    t = _inputs(g, d)
    neg = g.neg1.to(g.dev)
    for kw in ({"weighting": "mean"}, {"weighting": "edge"}, {"row_dtype": "bf16"}):
        want = _run(g, t.Ud, t.Pd, t.wd, neg, "edge", **kw)
        got = _run(g, t.Ud, t.Pd, t.wd, neg.reshape(-1, 1), "edge", **kw)
        for a, b, name in zip(got, want, ("loss", "dU", "dP")):
            assert torch.equal(a, b), (kw, name)
    # sample_negatives / draw_negatives: [E] as before, [E, k] for k > 1, the same values
    gen = torch.Generator(g.dev)
    one = ops.sample_negatives(g.ei_d, N_POSTS, gen.manual_seed(3))
    assert one.shape == (g.E,) and one.dtype == torch.int32
    assert torch.equal(one, ops.sample_negatives(g.ei_d, N_POSTS, gen.manual_seed(3), num_neg=1))
    three = ops.sample_negatives(g.ei_d, N_POSTS, gen.manual_seed(3), num_neg=3)
    assert three.shape == (g.E, 3) and three.dtype == torch.int32
    assert int(three.min()) >= 0 and int(three.max()) < N_POSTS
    draw = ops.draw_negatives(g.ei_d, N_POSTS, gen.manual_seed(3), num_neg=3)
    assert torch.equal(draw.tensor(), three)
