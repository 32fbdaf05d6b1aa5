"""bf16 row storage through the fused layer, the models and the loss (``row_dtype="bf16"`` /
``HGNN_ROW_DTYPE=bf16``): which rows the mode rounds, which it must not touch, and that the
gradients pass straight through the rounding.

Every comparison rounds the very tensor the layer under test receives: the fp32 reference runs
over extra node types ``user_b = R(user)``, ``post_b = R(post)`` that the relations gather from,
while the root segments stay on ``user`` / ``post``.  Same graph as test_row_bf16.py (300 users,
50 posts, degrees 0 / 64 / 65 / 700 / 300 at chunk 64) plus a random user <- user relation."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_USER, N_POST = 300, 50
CHUNK = 64
D, H = 64, 64


def close(got, ref):
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5 * scale)


def R(t):
    return t.to(torch.bfloat16).float()


class _RoundST(torch.autograd.Function):
    """R with a straight-through gradient."""

    @staticmethod
    def forward(ctx, x):
        return R(x)

    @staticmethod
    def backward(ctx, g):
        return g


def _edges():
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 13, N_USER)
    deg[0], deg[1], deg[2], deg[3], deg[200] = 0, 64, 65, 700, 300
    dst = np.repeat(np.arange(N_USER), deg)
    p = 1.0 / np.arange(1, N_POST + 1) ** 0.8
    src = rng.choice(N_POST, size=dst.size, p=p / p.sum())
    perm = rng.permutation(dst.size)
    uu = rng.integers(0, N_USER, size=(2, 2000))
    return (torch.from_numpy(np.stack([src[perm], dst[perm]])), torch.from_numpy(uu))


@pytest.fixture(scope="module")
def G():
    from truth_recommendation_gnn_amd.graph import RelationCSR
    dev = torch.device("cuda:0")
    pu, uu = _edges()
    pu, uu = pu.to(dev), uu.to(dev)
    up = pu.flip(0).contiguous()
    gen = torch.Generator().manual_seed(21)

    def rnd(*shape, s=1.0):
        return (s * torch.randn(*shape, generator=gen)).to(dev)

    return types.SimpleNamespace(
        dev=dev, ei_pu=pu, ei_uu=uu, ei_up=up,
        pu=RelationCSR(pu, N_POST, N_USER, chunk=CHUNK),     # user <- post
        uu=RelationCSR(uu, N_USER, N_USER, chunk=CHUNK),     # user <- user
        up=RelationCSR(up, N_USER, N_POST, chunk=CHUNK),     # post <- user
        user=rnd(N_USER, D), post=rnd(N_POST, D),
        w_user=rnd(H, 3 * D, s=0.1), b_user=rnd(H, s=0.1),
        w_post=rnd(H, 2 * D, s=0.1), b_post=rnd(H, s=0.1),
        g_user=rnd(N_USER, H), g_post=rnd(N_POST, H),
        neg=torch.randint(0, N_POST, (int(up.shape[1]),), generator=gen,
                          dtype=torch.int32).to(dev),
        pw=(0.5 + torch.rand(int(up.shape[1]), generator=gen)).to(dev))


def _leaf(t):
    return t.detach().clone().requires_grad_()


def _run(spec, xs, ws, G):
    from truth_recommendation_gnn_amd import ops
    out = ops.hetero_layer(spec, xs, ws)
    ((out["user"] * G.g_user).sum() + (out["post"] * G.g_post).sum()).backward()
    return out


def _specs(G, pre=()):
    """The layer in the mode over {user, post}, and its fp32 twin whose relations gather from
    the rounded copies {user_b, post_b}."""
    from truth_recommendation_gnn_amd import ops
    mode = ops.LayerSpec(("post", "user"), (
        ops.DstGroup("user", (("post", G.pu), ("user", G.uu)), True, True, pre),
        ops.DstGroup("post", (("user", G.up),), True, True)), "bf16")
    split = ops.LayerSpec(("post", "post_b", "user", "user_b"), (
        ops.DstGroup("user", (("post_b", G.pu), ("user_b", G.uu)), True, True),
        ops.DstGroup("post", (("user_b", G.up),), True, True)), "fp32")
    return mode, split


def test_layer_rounds_the_gathered_rows_and_passes_gradients_straight_through(G):
    mode, split = _specs(G)
    user, post = _leaf(G.user), _leaf(G.post)
    ws = [(_leaf(G.w_user), _leaf(G.b_user)), (_leaf(G.w_post), _leaf(G.b_post))]
    out = _run(mode, {"user": user, "post": post}, ws, G)

    user2, post2 = _leaf(G.user), _leaf(G.post)
    user_b, post_b = _leaf(R(G.user)), _leaf(R(G.post))
    ws2 = [(_leaf(G.w_user), _leaf(G.b_user)), (_leaf(G.w_post), _leaf(G.b_post))]
    ref = _run(split, {"user": user2, "post": post2, "user_b": user_b, "post_b": post_b}, ws2, G)

    for t in ("user", "post"):
        close(out[t], ref[t])
    close(user.grad, user2.grad + user_b.grad)
    close(post.grad, post2.grad + post_b.grad)
    for (w, b), (w2, b2) in zip(ws, ws2):
        close(w.grad, w2.grad)
        close(b.grad, b2.grad)
    # and the mode is engaged: the unrounded fp32 layer gives other numbers
    from truth_recommendation_gnn_amd import ops
    fp32 = ops.hetero_layer(ops.LayerSpec(mode.types, mode.groups, "fp32"),
                            {"user": G.user, "post": G.post},
                            [(G.w_user, G.b_user), (G.w_post, G.b_post)])
    assert not torch.equal(fp32["user"], out["user"].detach())


def test_pre_projected_rows_are_rounded_after_the_projection(G):
    from truth_recommendation_gnn_amd import ops
    mode, _ = _specs(G, pre=(True, False))
    user, post = _leaf(G.user), _leaf(G.post)
    ws = [(_leaf(G.w_user), _leaf(G.b_user)), (_leaf(G.w_post), _leaf(G.b_post))]
    out = _run(mode, {"user": user, "post": post}, ws, G)

    # by hand: P = post W^T -> R (straight through) -> mean; the user <- user and post <- user
    # relations gather R(user); roots, weights and the destination update are unrounded fp32
    u2, p2 = _leaf(G.user), _leaf(G.post)
    wu, bu, wp, bp = _leaf(G.w_user), _leaf(G.b_user), _leaf(G.w_post), _leaf(G.b_post)
    P = ops.fused_linear([p2], wu[:, :D].contiguous(), None, False)
    add = ops.mean_gather(_RoundST.apply(P), G.pu)
    ub = _RoundST.apply(u2)
    z = ops.fused_linear([ops.mean_gather(ub, G.uu), u2], wu[:, D:].contiguous(), bu, False) + add
    y_user = torch.relu(z)
    y_post = ops.fused_linear([ops.mean_gather(ub, G.up), p2], wp, bp, True)
    ((y_user * G.g_user).sum() + (y_post * G.g_post).sum()).backward()

    close(out["user"], y_user)
    close(out["post"], y_post)
    close(user.grad, u2.grad)
    close(post.grad, p2.grad)
    close(ws[0][0].grad, wu.grad)
    close(ws[0][1].grad, bu.grad)
    close(ws[1][0].grad, wp.grad)
    close(ws[1][1].grad, bp.grad)


# ----------------------------------------------------------------------------- left alone
def _both_modes(groups, types_, xs, ws, monkeypatch=None):
    """The layer's outputs and input gradients with row_dtype "bf16" and "fp32"."""
    from truth_recommendation_gnn_amd import ops
    res = []
    for mode in ("bf16", "fp32"):
        ops.clear_static_aggregates()
        x = {k: (_leaf(v) if v.requires_grad else v) for k, v in xs.items()}
        w = [(_leaf(a), _leaf(b)) for a, b in ws]
        out = ops.hetero_layer(ops.LayerSpec(types_, groups, mode), x, w)
        sum((o * o).sum() for o in out.values()).backward()
        res.append(([out[k].detach() for k in sorted(out)],
                    [x[k].grad for k in sorted(x) if x[k].requires_grad],
                    [a.grad for a, _ in w]))
    ops.clear_static_aggregates()
    return res


def _same(res):
    a, b = res
    for la, lb in zip(a, b):
        assert len(la) == len(lb)
        for ta, tb in zip(la, lb):
            assert torch.equal(ta, tb)


@pytest.mark.parametrize("static_agg", ("1", "0"))
def test_a_static_relation_keeps_fp32_rows(G, monkeypatch, static_agg):
    from truth_recommendation_gnn_amd import ops
    monkeypatch.setattr(ops, "STATIC_AGG", static_agg)
    groups = (ops.DstGroup("user", (("post", G.pu), ("user", G.uu)), True, True,
                           static=(True, True)),
              ops.DstGroup("post", (("user", G.up),), True, True, static=(True,)))
    _same(_both_modes(groups, ("post", "user"), {"user": G.user, "post": G.post},
                      [(G.w_user, G.b_user), (G.w_post, G.b_post)]))


def test_a_sampled_block_keeps_fp32_rows(G):
    from truth_recommendation_gnn_amd import ops
    from truth_recommendation_gnn_amd.graph import RelationCSR
    n_root = 100
    ei = G.ei_pu[:, G.ei_pu[1] < n_root].contiguous()
    uu = G.ei_uu[:, G.ei_uu[1] < n_root].contiguous()
    groups = (ops.DstGroup("user", (("post", RelationCSR(ei, N_POST, n_root)),
                                    ("user", RelationCSR(uu, N_USER, n_root))), True, True,
                           n_root=n_root),)
    _same(_both_modes(groups, ("post", "user"),
                      {"user": G.user.clone().requires_grad_(),
                       "post": G.post.clone().requires_grad_()}, [(G.w_user, G.b_user)]))


def test_a_width_that_is_no_multiple_of_8_keeps_fp32_rows(G):
    from truth_recommendation_gnn_amd import ops
    d = 20
    gen = torch.Generator().manual_seed(31)
    user = torch.randn(N_USER, d, generator=gen).to(G.dev).requires_grad_()
    post = torch.randn(N_POST, d, generator=gen).to(G.dev).requires_grad_()
    wu = (0.1 * torch.randn(32, 3 * d, generator=gen)).to(G.dev)
    wp = (0.1 * torch.randn(32, 2 * d, generator=gen)).to(G.dev)
    b = torch.zeros(32, device=G.dev)
    groups = (ops.DstGroup("user", (("post", G.pu), ("user", G.uu)), True, True),
              ops.DstGroup("post", (("user", G.up),), True, True))
    _same(_both_modes(groups, ("post", "user"), {"user": user, "post": post},
                      [(wu, b), (wp, b)]))


def test_an_explicit_fp32_is_the_default_path_whatever_the_module_says(G, monkeypatch):
    from truth_recommendation_gnn_amd import ops
    groups = (ops.DstGroup("user", (("post", G.pu), ("user", G.uu)), True, True),
              ops.DstGroup("post", (("user", G.up),), True, True))
    xs = {"user": G.user, "post": G.post}
    ws = [(G.w_user, G.b_user), (G.w_post, G.b_post)]
    want = ops.hetero_layer(ops.LayerSpec(("post", "user"), groups), xs, ws)
    bf = ops.hetero_layer(ops.LayerSpec(("post", "user"), groups, "bf16"), xs, ws)
    monkeypatch.setattr(ops, "ROW_DTYPE", "bf16")
    got = ops.hetero_layer(ops.LayerSpec(("post", "user"), groups, "fp32"), xs, ws)
    env = ops.hetero_layer(ops.LayerSpec(("post", "user"), groups), xs, ws)
    for t in ("user", "post"):
        assert torch.equal(got[t], want[t])
        assert torch.equal(env[t], bf[t])          # None is ops.ROW_DTYPE at call time
        assert not torch.equal(bf[t], want[t])
    with pytest.raises(ValueError, match="fp32.*bf16"):
        ops.hetero_layer(ops.LayerSpec(("post", "user"), groups, "fp16"), xs, ws)


# ----------------------------------------------------------------------------- plumbing
def test_model_keyword_and_module_switch_are_the_same_step(G, monkeypatch):
    from truth_recommendation_gnn_amd import HeteroSAGE, ops
    rels = [(("post", "rev_engages", "user"), 1.0), (("user", "social", "user"), 0.75),
            (("user", "engages", "post"), 1.0)]
    eid = {rels[0][0]: G.ei_pu, rels[1][0]: G.ei_uu, rels[2][0]: G.ei_up}
    xd = {"user": G.user, "post": G.post}
    torch.manual_seed(3)
    m_kw = HeteroSAGE(H, rels, num_layers=2, in_channels=D, row_dtype="bf16").to(G.dev)
    m_env = HeteroSAGE(H, rels, num_layers=2, in_channels=D).to(G.dev)
    m_env.load_state_dict(m_kw.state_dict())
    assert list(m_kw.state_dict()) == list(m_env.state_dict())
    with pytest.raises(ValueError, match="fp32.*bf16"):
        HeteroSAGE(H, rels, row_dtype="half")

    def step(model, loss_dtype):
        model.zero_grad(set_to_none=True)
        out = model(xd, eid)
        loss = ops.edge_bce_loss(out["user"], out["post"], G.ei_up, G.neg, G.pw,
                                 neg_order="user", row_dtype=loss_dtype)
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    ops.clear_static_aggregates()
    l_kw, g_kw = step(m_kw, "bf16")
    l_fp32, _ = step(m_env, None)                   # the module still says fp32
    monkeypatch.setattr(ops, "ROW_DTYPE", "bf16")
    l_env, g_env = step(m_env, None)
    ops.clear_static_aggregates()
    assert torch.equal(l_kw, l_env)
    assert g_kw.keys() == g_env.keys() and len(g_kw) > 0
    for n in g_kw:
        assert torch.equal(g_kw[n], g_env[n]), n
    assert not torch.equal(l_kw, l_fp32)            # the mode is engaged (layer 2 and the loss)
