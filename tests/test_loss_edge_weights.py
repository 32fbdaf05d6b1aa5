"""Per-edge positive weights in the fused link loss (``weighting="edge"``).

    loss = mean_e( w_e * softplus(-<U[u_e], P[p_e]>) ) + mean_e softplus(<U[u_e], P[n_e]>)

against float64 autograd of that expression written out here, on every row format the two loss
kernels read (fp32, bf16, zero-packed fp32) and every form of negatives (int64 in edge order, int32
in user order, a ``NegativeDraw``).

Shapes, as ``tests/test_zpack.py`` builds its graph: 300 users, 37 posts, about 3000 positive edges
in shuffled COO order (both permutations non-trivial); one user with 130 positives (three 64-edge
batches of the scoring pass, the last partial) and one with none; one post with 200 positives
(above the default chunk of 64: weighted chunks go through the slab and the fixup), one without
positives, one without negatives.  Widths: those of ``test_edge_bce_loss_matches_oracle`` plus 8,
the narrowest bf16 row.

Weights: 3.0 where the float64 positive score of the edge lies below the median, else 1.0.
Independent random weights move the loss by about the tolerance itself; these, correlated with
the score, move it by several percent, which test 1 asserts before it compares.

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
DS = (64, 128, 5, 200, 16, 8)
DS_BF16 = tuple(d for d in DS if d % 8 == 0)
DS_ZP = (64, 128)
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


def _scores64(U, P, ei):
    return (U.double()[ei[0]] * P.double()[ei[1]]).sum(1)


def _weights(U, P, ei):
    s = _scores64(U, P, ei)
    return torch.where(s < s.median(), 3.0, 1.0).float()


def _ref64(U, P, ei, neg, w, weighting="edge"):
    """float64 autograd of the loss written out: (loss, dU, dP) for the upstream gradient UP."""
    Ur, Pr = U.double().requires_grad_(), P.double().requires_grad_()
    u = Ur[ei[0]]
    sp, sn = (u * Pr[ei[1]]).sum(1), (u * Pr[neg]).sum(1)
    neg_loss = BCE(sn, torch.zeros_like(sn))
    if weighting == "edge":
        loss = (w.double() * BCE(sp, torch.ones_like(sp), reduction="none")).mean() + neg_loss
    else:
        loss = (w.double() * BCE(sp, torch.ones_like(sp))).mean() + neg_loss
    (loss * UP).backward()
    return loss.detach(), Ur.grad, Pr.grad


# ----------------------------------------------------------------------------- CPU
def test_link_loss_edge_is_the_per_edge_sum():
    user, post, neg = _graph()
    ei, neg = torch.from_numpy(np.stack([user, post])), torch.from_numpy(neg)
    U, P = (t.double() for t in _tables(8))
    w = _weights(U, P, ei).double()
    got = ops.link_loss(U, P, ei, neg, w, weighting="edge")
    sp, sn = _scores64(U, P, ei), _scores64(U, P, torch.stack([ei[0], neg]))
    want = 0.0
    for e in range(ei.shape[1]):                           # the explicit per-edge loop
        want += float(w[e]) * float(np.logaddexp(0.0, -float(sp[e])))
        want += float(np.logaddexp(0.0, float(sn[e])))
    want /= ei.shape[1]
    assert abs(float(got) - want) <= 1e-12 * abs(want)
    mean = ops.link_loss(U, P, ei, neg, w, weighting="mean")
    assert torch.equal(mean, ops.link_loss(U, P, ei, neg, w))          # the default
    assert abs(float(got) - float(mean)) > 1e-2 * abs(float(mean))     # non-constant weights
    c = torch.full_like(w, 1.75)
    a, b = (ops.link_loss(U, P, ei, neg, c, weighting=m) for m in ("edge", "mean"))
    assert abs(float(a) - float(b)) <= 1e-14 * abs(float(b))           # constant weights
    with pytest.raises(ValueError, match="weighting"):
        ops.link_loss(U, P, ei, neg, w, weighting="sum")


def test_argument_errors_that_need_no_device():
    user, post, neg = _graph()
    ei, neg = torch.from_numpy(np.stack([user, post])), torch.from_numpy(neg)
    U, P = _tables(8)
    w = torch.ones(ei.shape[1])
    one = torch.ones(())
    with pytest.raises(ValueError, match="weighting='max'"):
        ops.edge_bce_loss(U, P, ei, neg, w, weighting="max")
    with pytest.raises(ValueError, match="weighting='max'"):
        ops.edge_bce_loss_raw(U, P, ei, neg, ei.shape[1], one, weighting="max")
    with pytest.raises(ValueError, match="needs pos_weights"):
        ops.edge_bce_loss(U, P, ei, neg, None, weighting="edge")
    with pytest.raises(ValueError, match="needs pos_weights"):
        ops.edge_bce_loss(U, P, ei, neg, w[:-1], weighting="edge")
    with pytest.raises(ValueError, match="needs pos_weights"):
        ops.edge_bce_loss(U, P, ei, neg, one, weighting="edge")            # the collapsed scalar
    for kw in ({"cscale": one}, {"n_edges_total": 2 * ei.shape[1]}, {"ready": lambda: None}):
        with pytest.raises(ValueError, match="does not combine with " + next(iter(kw))):
            ops.edge_bce_loss(U, P, ei, neg, w, weighting="edge", **kw)
    with pytest.raises(ValueError, match="does not combine with cscale / n_edges_total"):
        ops.edge_bce_loss_raw(U, P, ei, neg, ei.shape[1], one, pos_weights=w, weighting="edge")
    for kw in ({"ready": lambda: None}, {"on_dP": lambda dP: None},
               {"p_chunks": [(0, N_POSTS, None)]}):
        with pytest.raises(ValueError, match="does not combine with " + next(iter(kw))):
            ops.edge_bce_loss_raw(U, P, ei, neg, None, None, pos_weights=w, weighting="edge",
                                  **kw)
    with pytest.raises(ValueError, match="needs n_edges_total and cscale"):
        ops.edge_bce_loss_raw(U, P, ei, neg, None, None)


def test_new_entries_check_edge_w_and_widths_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_int64 * 4)()
    x = ctypes.c_void_p(ctypes.addressof(buf))     # non-null, never dereferenced: the checks
    #                                                below all fail before a launch
    for name, bad_d in (("hgnn_score_gather2_w", None), ("hgnn_score_gather2_w_zp", 96),
                        ("hgnn_score_gather2_w_bf16", 12)):
        fn = getattr(lib, name)

        def call(d, edge_w, rowptr_n=x, n_rows=5):
            return fn(x, 10, x, d, x, x, edge_w, rowptr_n, x, n_rows, x, 1.0, None, None, 0, 0,
                      64, None, x, None)

        assert call(128, None) == HGNN_E_ARG
        assert b"edge_w is null" in lib.hgnn_last_error_string()
        assert name[5:].encode() in lib.hgnn_last_error_string()
        assert call(128, None, rowptr_n=None) == HGNN_E_ARG
        assert b"rowptr_n is null" in lib.hgnn_last_error_string()
        assert call(128, None, n_rows=0) == 0                  # no rows: nothing to weigh
        if bad_d is not None:
            assert call(bad_d, x) == HGNN_E_UNSUPPORTED
            assert b"d=%d" % bad_d in lib.hgnn_last_error_string()
    for name, bad_d in (("hgnn_edge_score_fwd_w", 513), ("hgnn_edge_score_fwd_w_bf16", 12)):
        fn = getattr(lib, name)

        def call(d, edge_w, negs=(x, None, None)):
            return fn(x, x, d, 4, 9, x, x, edge_w, *negs, 10, x, x, x, x, None, None)

        assert call(64, None) == HGNN_E_ARG
        assert b"edge_w is null" in lib.hgnn_last_error_string()
        assert call(64, x, (x, x, None)) == HGNN_E_ARG
        assert b"exactly one form" in lib.hgnn_last_error_string()
        assert call(64, x, (None, None, None)) == HGNN_E_ARG
        assert call(bad_d, x) == HGNN_E_UNSUPPORTED
        assert b"d=%d" % bad_d in lib.hgnn_last_error_string()


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def g():
    user, post, neg = _graph()
    dev = torch.device("cuda:0")
    ei = torch.from_numpy(np.stack([user, post]))
    ei_d = ei.to(dev)
    csr = ops.relation_csr_for_loss(ei_d, N_USERS, N_POSTS)
    assert csr.fwd.plan.n_heavy > 0                         # the 200-edge post is split
    perm_u, perm_p = csr.bwd.perm.cpu().long(), csr.fwd.perm.cpu().long()
    ident = torch.arange(ei.shape[1])
    assert not torch.equal(perm_u, ident) and not torch.equal(perm_p, ident)
    rp_u = csr.bwd.rowptr.cpu()
    assert int(rp_u[BIG_USER + 1] - rp_u[BIG_USER]) == 130
    assert int(rp_u[NO_EDGE_USER + 1] - rp_u[NO_EDGE_USER]) == 0
    neg = torch.from_numpy(neg)
    # the three forms: int64 in edge order, the same draws as int32 in user order, and a draw
    draw = ops.draw_negatives(ei_d, N_POSTS)
    neg_draw = torch.empty(ei.shape[1], dtype=torch.int64)
    neg_draw[perm_u] = draw.tensor().cpu().long()           # back to edge order, for the reference
    forms = {"i64_edge": (neg.to(dev), "edge", neg),
             "i32_user": (neg[perm_u].to(torch.int32).to(dev), "user", neg),
             "draw": (draw, "user", neg_draw)}
    return types.SimpleNamespace(dev=dev, ei=ei, ei_d=ei_d, csr=csr, E=int(ei.shape[1]),
                                 forms=forms)


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


def _ref(g, t, form, weighting="edge"):
    key = (form, weighting)
    if key not in t.ref:
        t.ref[key] = _ref64(t.U, t.P, g.ei, g.forms[form][2], t.w, weighting)
    return t.ref[key]


def _run(g, U, P, w, form="i64_edge", **kw):
    """edge_bce_loss + backward with the upstream gradient UP: (loss, dU, dP)."""
    neg, order, _ = g.forms[form]
    U, P = U.clone().requires_grad_(), P.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, neg, w, neg_order=order, **kw)
    (loss * UP).backward()
    return loss.detach(), U.grad, P.grad


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["i64_edge", "i32_user", "draw"])
@pytest.mark.parametrize("d", DS)
def test_per_edge_loss_matches_float64(g, d, form):
    t = _inputs(g, d)
    ref = _ref(g, t, form)
    collapsed = _ref(g, t, form, "mean")
    tol = RTOL * abs(float(ref[0])) + ATOL_SCALE * abs(float(ref[0]))
    assert abs(float(ref[0]) - float(collapsed[0])) > 100 * tol     # the weighting is visible
    got = _run(g, t.Ud, t.Pd, t.wd, form, weighting="edge")
    for a, b, name in zip(got, ref, ("loss", "dU", "dP")):
        print(name, float((a.double().cpu() - b).abs().max()), float(b.abs().max()))
        close(a, b)
    assert float(got[2][HEAVY].abs().max()) > 0 and float(got[2][NO_POS].abs().max()) > 0
    assert float(got[1][NO_EDGE_USER].abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
def test_constant_weights_are_bitwise_the_collapsed_loss(g, d):
    """A power of two commutes with every rounding: any difference is a changed lane layout or
    summation order."""
    t = _inputs(g, d)
    w = torch.full((g.E,), 2.0, device=g.dev)
    for form in g.forms:
        want = _run(g, t.Ud, t.Pd, w, form, weighting="mean")
        got = _run(g, t.Ud, t.Pd, w, form, weighting="edge")
        for a, b, name in zip(got, want, ("loss", "dU", "dP")):
            assert torch.equal(a, b), (form, name)


def _timed_names(fn):
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        res = fn()
    finally:
        ops.set_timer(None)
    return res, timer.records


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS_ZP)
def test_zero_packed_rows_are_bitwise_the_unpacked_rows(g, d, monkeypatch):
    t = _inputs(g, d, relu=True)
    assert 0.3 < float((t.U == 0).float().mean()) < 0.7
    neg, order, _ = g.forms["i64_edge"]

    def run():
        return ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, neg, None, None, neg_order=order,
                                     pos_weights=t.wd, weighting="edge")

    monkeypatch.setenv("HGNN_ZPACK", "0")
    want, rec0 = _timed_names(run)
    monkeypatch.setenv("HGNN_ZPACK", "1")
    got, rec1 = _timed_names(run)
    names0, names1 = [r[0] for r in rec0], [r[0] for r in rec1]
    assert not any(n.startswith("zpack[") for n in names0)
    assert f"zpack[{N_USERS}]x{d}" in names1                    # the pack pass ran
    for n in (f"score_gather[{N_POSTS}<-{N_USERS}]x{d}", f"edge_score_d{d}"):
        assert n in names0 and n in names1                      # the entries keep their names
    for a, b, name in zip(got, want, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name
    ref = _ref(g, t, "i64_edge")                                # and both are the weighted loss
    close(got[0], ref[0])
    close(got[2] * UP, ref[2])


@pytest.mark.gpu
def test_timer_counts_the_weights_bytes(g):
    t = _inputs(g, 64)
    neg, order, _ = g.forms["i64_edge"]
    recs = []
    for kw in ({"n_edges_total": g.E, "cscale": t.wd.mean()},
               {"n_edges_total": None, "cscale": None, "pos_weights": t.wd, "weighting": "edge"}):
        _, r = _timed_names(lambda: ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, neg,
                                                          neg_order=order, **kw))
        recs.append({x[0]: x for x in r})
    for name in (f"score_gather[{N_POSTS}<-{N_USERS}]x64", "edge_score_d64"):
        assert recs[1][name][1] - recs[0][name][1] == 4 * g.E   # 4 B per positive edge


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS_BF16)
def test_bf16_rows(g, d):
    t = _inputs(g, d)
    Ur, Pr = ops.rows_to_bf16(t.Ud).float(), ops.rows_to_bf16(t.Pd).float()
    want = _run(g, Ur, Pr, t.wd, weighting="edge", row_dtype="fp32")
    got = _run(g, t.Ud, t.Pd, t.wd, weighting="edge", row_dtype="bf16")
    for a, b in zip(got, want):
        close(a, b)
    again = _run(g, t.Ud, t.Pd, t.wd, weighting="edge", row_dtype="bf16")
    for a, b, name in zip(again, got, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name
    # the draw and the int32 negatives reach the bf16 entry too
    for form in ("i32_user", "draw"):
        Ub, Pb = Ur.cpu(), Pr.cpu()
        ref = _ref64(Ub, Pb, g.ei, g.forms[form][2], t.w)
        for a, b in zip(_run(g, t.Ud, t.Pd, t.wd, form, weighting="edge", row_dtype="bf16"), ref):
            close(a, b)


@pytest.mark.gpu
def test_in_place_change_of_the_weights_and_retained_graph(g):
    d = 64
    t = _inputs(g, d)
    w = t.wd.clone()
    close(_run(g, t.Ud, t.Pd, w, weighting="edge")[2], _ref(g, t, "i64_edge")[2])
    first = g.csr._edge_w[2]
    _run(g, t.Ud, t.Pd, w, weighting="edge")
    assert g.csr._edge_w[2] is first                    # the same weights: no new permutation
    w.mul_(-1).add_(4)                                  # 3 <-> 1, in place
    ref = _ref64(t.U, t.P, g.ei, g.forms["i64_edge"][2], 4 - t.w)
    assert abs(float(ref[0]) - float(_ref(g, t, "i64_edge")[0])) > 1e-2 * abs(float(ref[0]))
    for a, b in zip(_run(g, t.Ud, t.Pd, w, weighting="edge"), ref):
        close(a, b)
    assert g.csr._edge_w[2] is not first
    # a second backward through a retained graph returns what the first did, whatever became
    # of the caller's weights in between
    neg, order, _ = g.forms["i64_edge"]
    U, P = t.Ud.clone().requires_grad_(), t.Pd.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, neg, w, neg_order=order, weighting="edge")
    (loss * UP).backward(retain_graph=True)
    g1 = (U.grad.clone(), P.grad.clone())
    U.grad = P.grad = None
    w.fill_(1.0)
    (loss * UP).backward()
    assert torch.equal(U.grad, g1[0]) and torch.equal(P.grad, g1[1])
    close(g1[0], ref[1])


@pytest.mark.gpu
def test_errors_on_the_device(g):
    d = 64
    t = _inputs(g, d)
    neg, order, _ = g.forms["i64_edge"]
    lib, pf = N.lib(), g.csr.fwd
    rowptr_n = torch.zeros(N_POSTS + 1, dtype=torch.int32, device=g.dev)
    col_n = torch.zeros(1, dtype=torch.int32, device=g.dev)
    out = torch.zeros(N_POSTS, d, device=g.dev)
    c = torch.ones((), device=g.dev)
    rc = lib.hgnn_score_gather2_w(
        N.ptr(t.Ud), N_USERS, N.ptr(t.Pd), d, N.ptr(pf.rowptr), N.ptr(pf.col), None,
        N.ptr(rowptr_n), N.ptr(col_n), N_POSTS, N.ptr(c), 1.0 / g.E,
        *ops._plan_args(pf.plan, d, g.dev), N.ptr(out), N.stream_ptr(g.dev))
    assert rc == HGNN_E_ARG and b"edge_w is null" in lib.hgnn_last_error_string()
    assert float(out.abs().max()) == 0                  # refused before any launch
    with pytest.raises(ValueError, match="p_chunks"):
        ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, neg, None, None, neg_order=order,
                              p_chunks=[(0, N_POSTS, None)], pos_weights=t.wd, weighting="edge")
    with pytest.raises(ValueError, match="cscale"):
        ops.edge_bce_loss(t.Ud, t.Pd, g.ei_d, neg, t.wd, neg_order=order, weighting="edge",
                          cscale=c)
    with pytest.raises(ValueError, match="weighting"):
        ops.edge_bce_loss(t.Ud, t.Pd, g.ei_d, neg, t.wd, neg_order=order, weighting="Edge")


@pytest.mark.gpu
@pytest.mark.parametrize("d", (64, 5))
def test_default_is_the_collapsed_weighting(g, d):
    t = _inputs(g, d)
    want = _run(g, t.Ud, t.Pd, t.wd, weighting="mean")
    got = _run(g, t.Ud, t.Pd, t.wd)
    for a, b, name in zip(got, want, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name
    close(got[0], _ref(g, t, "i64_edge", "mean")[0])
