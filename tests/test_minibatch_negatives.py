"""The mini-batch link loss with k weighted negatives, per-edge weights and logQ
(``minibatch.LinkLoss`` / ``link_batch`` / ``LinkSampler`` options; ``hgnn_link_seeds_k``,
``hgnn_link_group_k``).  The small setup is ``test_minibatch_graph.py``'s (copied, not imported:
48 positives, fanouts (5, 3), ``slack=16``)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HGNN_E_ARG = 1001


# ----------------------------------------------------------------------------- hgnn_link_seeds_k
def _seed_inputs(B, k, id_range, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    M = 3 * B
    src = torch.randint(0, id_range, (M,), device=DEV, generator=gen)
    dst = torch.randint(0, id_range, (M,), device=DEV, generator=gen)
    eid = torch.randperm(M, device=DEV, generator=gen)[:B].contiguous()
    neg = torch.randint(0, id_range, (B, k), device=DEV, generator=gen)
    return src, dst, eid, neg


def _run_seeds_k(src, dst, eid, neg, B, k):
    from truth_recommendation_gnn_amd import _native as N
    i32 = dict(dtype=torch.int32, device=DEV)
    out = {n: torch.full((m,), -7, **i32) for n, m in (
        ("seeds_u", B), ("seeds_p", B * (1 + k)), ("pu", B), ("pp", B), ("pn", B * k),
        ("counts", 2))}
    is32 = neg.dtype == torch.int32
    rc = N.lib().hgnn_link_seeds_k(
        N.ptr(src), N.ptr(dst), N.ptr(eid), None if is32 else N.ptr(neg),
        N.ptr(neg) if is32 else None, B, k,
        *[N.ptr(out[n]) for n in ("seeds_u", "seeds_p", "pu", "pp", "pn", "counts")],
        N.stream_ptr(DEV))
    return rc, out


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("B,k,id_range", [(48, 3, 50_000), (1024, 3, 50_000),
                                          (1024, 4, 50_000), (2048, 7, 50_000), (300, 2, 40)])
def test_link_seeds_k_equals_unique_and_searchsorted(B, k, id_range, dtype):
    """Cases a-e of the seed kernel (192 keys; the old cap of 4,096; the first size past it;
    the new cap of 16,384 keys = 128 KiB of LDS; ids from a range of 40, nearly all duplicates),
    int64 and int32 negatives: seeds, counts and local ids against torch.unique +
    searchsorted, and nothing written past the counts (outputs pre-filled with -7)."""
    src, dst, eid, neg = _seed_inputs(B, k, id_range, 11 * B + k)
    neg = neg.to(dtype).contiguous()
    rc, out = _run_seeds_k(src, dst, eid, neg, B, k)
    assert rc == 0
    pos_u, pos_p = src[eid], dst[eid]
    su = torch.unique(pos_u)
    sp = torch.unique(torch.cat([pos_p, neg.reshape(-1).long()]))
    nu, np_ = int(su.numel()), int(sp.numel())
    assert out["counts"].tolist() == [nu, np_]
    assert torch.equal(out["seeds_u"][:nu].long(), su)
    assert torch.equal(out["seeds_p"][:np_].long(), sp)
    assert bool((out["seeds_u"][nu:] == -7).all()) and bool((out["seeds_p"][np_:] == -7).all())
    assert torch.equal(out["pu"].long(), torch.searchsorted(su, pos_u))
    assert torch.equal(out["pp"].long(), torch.searchsorted(sp, pos_p))
    assert torch.equal(out["pn"].view(B, k).long(), torch.searchsorted(sp, neg.long()))


@pytest.mark.parametrize("B", [48, 1024])
def test_link_seeds_k_with_one_negative_equals_link_seeds(B):
    from truth_recommendation_gnn_amd import _native as N
    src, dst, eid, neg = _seed_inputs(B, 1, 5_000, B)
    rc, got = _run_seeds_k(src, dst, eid, neg, B, 1)
    assert rc == 0
    i32 = dict(dtype=torch.int32, device=DEV)
    want = {n: torch.full((m,), -7, **i32) for n, m in (
        ("seeds_u", B), ("seeds_p", 2 * B), ("pu", B), ("pp", B), ("pn", B), ("counts", 2))}
    N.check(N.lib().hgnn_link_seeds(
        N.ptr(src), N.ptr(dst), N.ptr(eid), N.ptr(neg.reshape(-1)), B,
        *[N.ptr(want[n]) for n in ("seeds_u", "seeds_p", "pu", "pp", "pn", "counts")],
        N.stream_ptr(DEV)), "hgnn_link_seeds")
    for n in want:
        assert torch.equal(got[n], want[n]), n


def test_link_seeds_k_refuses_more_than_its_capacity():
    src, dst, eid, neg = _seed_inputs(2048, 8, 50_000, 3)
    rc, out = _run_seeds_k(src, dst, eid, neg, 2048, 8)
    assert rc == HGNN_E_ARG
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out.values())      # refused before any launch


# ----------------------------------------------------------------------------- hgnn_link_group_k
_NINE = ("rowptr", "col", "neg", "uop", "p_rowptr", "p_users", "p_perm", "n_rowptr", "n_users")


def _run_group_k(pu, pp, pn, E, nu, np_, k, w=None, logq=None, seeds_p=None, count=None):
    from truth_recommendation_gnn_amd import _native as N
    i32 = dict(dtype=torch.int32, device=DEV)
    out = {n: torch.full((m,), -7, **i32) for n, m in (
        ("rowptr", nu + 1), ("col", E), ("neg", E * k), ("uop", E), ("p_rowptr", np_ + 1),
        ("p_users", E), ("p_perm", E), ("n_rowptr", np_ + 1), ("n_users", E * k))}
    f32 = dict(dtype=torch.float32, device=DEV)
    out["w_user"] = torch.full((E,), -7.0, **f32) if w is not None else None
    out["w_post"] = torch.full((E,), -7.0, **f32) if w is not None else None
    out["logq"] = torch.full((np_,), -7.0, **f32) if logq is not None else None
    ws = torch.empty(int(N.lib().hgnn_link_group_k_ws_bytes(E, k)), dtype=torch.uint8,
                     device=DEV)
    N.check(N.lib().hgnn_link_group_k(
        N.ptr(pu), N.ptr(pp), N.ptr(pn), N.ptr(w), N.ptr(logq), N.ptr(seeds_p),
        int(seeds_p.numel()) if seeds_p is not None else 0, N.ptr(count), E, k, nu, np_,
        *[N.ptr(out[n]) for n in _NINE], N.ptr(out["w_user"]), N.ptr(out["w_post"]),
        N.ptr(out["logq"]), N.ptr(ws), ws.numel(), N.stream_ptr(DEV)), "hgnn_link_group_k")
    return out


@pytest.mark.parametrize("opts", [False, True])
@pytest.mark.parametrize("E,nu,np_,k", [(48, 48, 192, 3), (1024, 1024, 5120, 4),
                                        (3000, 2500, 9100, 2)])
def test_link_group_k_equals_torch_grouping(E, nu, np_, k, opts):
    """hgnn_link_group_k against the torch grouping (stable argsorts): the pairs by user, row p
    of ``neg`` the negatives of user-grouped position p, the same pairs by post, all E·k
    (negative, user) pairs by post; with ``opts`` the weights in both kernel orders and the local
    logQ table, exact gathers (``torch.equal``), rows past the seeds 0 — the seeds' count given
    by the array's length and, at the same values, by a device counter over a full-capacity
    array."""
    gen = torch.Generator(device=DEV).manual_seed(E + k)
    pu = torch.randint(0, nu, (E,), device=DEV, generator=gen, dtype=torch.int32)
    pp = torch.randint(0, np_, (E,), device=DEV, generator=gen, dtype=torch.int32)
    pn = torch.randint(0, np_, (E, k), device=DEV, generator=gen, dtype=torch.int32)
    w = logq = seeds_p = None
    if opts:
        G, n_seeds = 3 * np_, np_ - 7
        w = torch.rand(E, device=DEV, generator=gen) + 0.5
        logq = -torch.rand(G, device=DEV, generator=gen) * 9
        seeds_p = torch.randint(0, G, (n_seeds,), device=DEV, generator=gen, dtype=torch.int32)
    out = _run_group_k(pu, pp, pn, E, nu, np_, k, w, logq, seeds_p)
    order = torch.argsort(pu.long(), stable=True)
    rowptr = torch.zeros(nu + 1, dtype=torch.long, device=DEV)
    rowptr[1:] = torch.cumsum(torch.bincount(pu.long(), minlength=nu), 0)
    col, neg, uop = pp[order], pn[order], pu[order]
    assert torch.equal(out["rowptr"].long(), rowptr)
    assert torch.equal(out["col"], col) and torch.equal(out["neg"].view(E, k), neg)
    assert torch.equal(out["uop"], uop)
    po = torch.argsort(col.long(), stable=True)
    prow = torch.zeros(np_ + 1, dtype=torch.long, device=DEV)
    prow[1:] = torch.cumsum(torch.bincount(col.long(), minlength=np_), 0)
    assert torch.equal(out["p_rowptr"].long(), prow)
    assert torch.equal(out["p_perm"].long(), po) and torch.equal(out["p_users"], uop[po])
    flat = neg.reshape(-1).long()
    no = torch.argsort(flat, stable=True)
    nrow = torch.zeros(np_ + 1, dtype=torch.long, device=DEV)
    nrow[1:] = torch.cumsum(torch.bincount(flat, minlength=np_), 0)
    assert torch.equal(out["n_rowptr"].long(), nrow)
    assert torch.equal(out["n_users"], uop.repeat_interleave(k)[no])
    if opts:
        assert torch.equal(out["w_user"], w[order])
        assert torch.equal(out["w_post"], w[order][po])
        want = torch.zeros(np_, device=DEV)
        want[:n_seeds] = logq[seeds_p.long()]
        assert torch.equal(out["logq"], want)
        # the same table from a full-capacity seed array (valid ids after the count, as a
        # LinkSampler's buffer holds) and the count on the device
        full = torch.cat([seeds_p, torch.full((7,), 5, dtype=torch.int32, device=DEV)])
        cnt = torch.tensor([n_seeds], dtype=torch.int32, device=DEV)
        again = _run_group_k(pu, pp, pn, E, nu, np_, k, w, logq, full, cnt)
        for n in out:
            assert torch.equal(again[n], out[n]), n


@pytest.mark.parametrize("E,nu,np_", [(48, 48, 96), (1024, 1024, 2048)])
def test_link_group_k_with_one_negative_equals_link_group(E, nu, np_):
    from truth_recommendation_gnn_amd import _native as N
    gen = torch.Generator(device=DEV).manual_seed(E)
    pu = torch.randint(0, nu, (E,), device=DEV, generator=gen, dtype=torch.int32)
    pp = torch.randint(0, np_, (E,), device=DEV, generator=gen, dtype=torch.int32)
    pn = torch.randint(0, np_, (E,), device=DEV, generator=gen, dtype=torch.int32)
    got = _run_group_k(pu, pp, pn, E, nu, np_, 1)
    want = {n: torch.full_like(got[n], -7) for n in _NINE}
    ws = torch.empty(int(N.lib().hgnn_link_group_ws_bytes(E)), dtype=torch.uint8, device=DEV)
    N.check(N.lib().hgnn_link_group(
        N.ptr(pu), N.ptr(pp), N.ptr(pn), E, nu, np_, *[N.ptr(want[n]) for n in _NINE],
        N.ptr(ws), ws.numel(), N.stream_ptr(DEV)), "hgnn_link_group")
    for n in _NINE:
        assert torch.equal(got[n], want[n]), n


# ----------------------------------------------------------------------------- the Python path
def _link_setup(B=48, fanouts=(5, 3)):
    """test_minibatch_graph.py's graph, sampler and model (cfg5 x 0.0002, d = 16)."""
    from truth_recommendation_gnn_amd import HeteroSAGE, sampler, synth
    cfg = synth.dataclasses.replace(synth.scaled("cfg5", 0.0002), dim=16, hidden=16)
    g = synth.make_graph(cfg, device=DEV)
    rels = [(synth.REV_ENGAGES, 1.0), (synth.SOCIAL, 0.75), (synth.ENGAGES, 1.0),
            (synth.POST_POST, 0.5)]
    num = {"user": cfg.num_users, "post": cfg.num_posts}
    s = sampler.NeighborSampler(num, g.edge_index_dict, [et for et, _ in rels], list(fanouts))

    def make_model():
        torch.manual_seed(synth.WEIGHT_SEED)
        return HeteroSAGE(cfg.hidden, rels, num_layers=2, in_channels=cfg.dim).to(DEV)

    ei = g.edge_index_dict[synth.ENGAGES]
    return g, s, make_model, ei, cfg.num_users, cfg.num_posts, B


def _close(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / max(scale, 1e-30)
    assert err < 1e-4, (what, err)


def _options(setting, ei, U, P):
    """(LinkLoss keywords, link_batch / LinkSampler keywords, k) of a named setting."""
    from truth_recommendation_gnn_amd import metrics, ops
    if setting == "k3_uniform":
        return {"num_neg": 3}, {}, 3
    if setting == "k3_weighted_avoid":
        return {"num_neg": 3}, {"distribution": ops.PostDistribution.from_degree(ei, P),
                                "avoid": metrics.SeenIndex(ei, U, P)}, 3
    if setting == "k2_edge_logq":
        gen = torch.Generator(device=DEV).manual_seed(3)
        w = torch.randint(0, 2, (int(ei.shape[1]),), device=DEV, generator=gen).float() * 2 + 1
        logq = ops.PostDistribution.from_degree(ei, P).log_q(2)
        return {"num_neg": 2, "weighting": "edge", "logq": logq}, {"pos_weights": w}, 2
    if setting == "all":
        dist = ops.PostDistribution.from_degree(ei, P)
        gen = torch.Generator(device=DEV).manual_seed(3)
        w = torch.randint(0, 2, (int(ei.shape[1]),), device=DEV, generator=gen).float() * 2 + 1
        return ({"num_neg": 3, "weighting": "edge", "logq": dist.log_q(3)},
                {"distribution": dist, "avoid": metrics.SeenIndex(ei, U, P), "pos_weights": w}, 3)
    raise AssertionError(setting)


@pytest.mark.parametrize("setting", ["k3_uniform", "k3_weighted_avoid", "k2_edge_logq"])
def test_link_sampler_stages_what_the_eager_path_stages(setting):
    """``LinkSampler.prepare`` against ``link_batch`` (same arguments, same generator seed) +
    ``NeighborSampler.sample`` + ``CapturedStep.prepare(mb, pu, pp, pn, w, seeds_p)``: every byte
    of the blocks' and the loss's arenas, and the sampled edge count."""
    from truth_recommendation_gnn_amd import minibatch
    g, s, make_model, ei, U, P, B = _link_setup()
    lkw, skw, k = _options(setting, ei, U, P)
    n_seeds = {"user": B, "post": (1 + k) * B}
    ll = minibatch.LinkLoss(B, n_seeds["user"], n_seeds["post"], DEV, **lkw)
    step = minibatch.CapturedStep(make_model(), g.x_dict, s, n_seeds, ll, None, slack=16)
    ls = minibatch.LinkSampler(step, ei, P, **skw)
    order = torch.randperm(int(ei.shape[1]), device=DEV,
                           generator=torch.Generator(device=DEV).manual_seed(7))
    barena, larena = step.blocks.arena._bytes["stage"], ll.arena._bytes["stage"]
    for b in range(3):
        ids = order[b * B:(b + 1) * B]
        lb = minibatch.link_batch(ei, ids, P, torch.Generator(device=DEV).manual_seed(100 + b),
                                  k, **skw)
        assert tuple(lb.pn.shape) == (B, k) and (lb.w is not None) == ("pos_weights" in skw)
        lb.mb = s.sample(lb.seeds, seed=b)
        step.prepare(lb.mb, lb.pu, lb.pp, lb.pn, lb.w,
                     lb.seeds["post"] if "logq" in lkw else None)
        want_b, want_l = barena.clone(), larena.clone()
        barena.fill_(0x5A)
        larena.fill_(0x5A)
        ls.prepare(ids, b, torch.Generator(device=DEV).manual_seed(100 + b))
        torch.cuda.synchronize()
        for name, (o, n, dt, nb) in step.blocks.arena.layout.items():
            assert torch.equal(barena[o:o + nb], want_b[o:o + nb]), (b, name)
        for name, (o, n, dt, nb) in ll.arena.layout.items():
            assert torch.equal(larena[o:o + nb], want_l[o:o + nb]), (b, name)
        assert int(ls.edge_count()) == sum(c.num_edges for blk in lb.mb.blocks
                                           for c in blk.csr.values())
        if "distribution" in skw:
            assert lb.neg_p.dtype == torch.int32 and int(lb.neg_p.max()) < P


def test_captured_step_with_every_option_matches_the_torch_loss():
    """The captured step with k = 3 popularity-weighted, seen-avoiding negatives, per-edge
    weights in {1, 3} and logQ = ``dist.log_q(3)``: captured on batch 0, replayed on three later
    batches staged by the ``LinkSampler``; loss (2e-6 relative) and every parameter gradient
    (``_close``) against ``sampler.forward_blocks`` + ``ops.link_loss(..., weighting="edge",
    logq=logq[seeds_p])`` on the same batch; two replays of one staged batch bitwise equal."""
    from truth_recommendation_gnn_amd import minibatch, ops, sampler
    g, s, make_model, ei, U, P, B = _link_setup()
    lkw, skw, k = _options("all", ei, U, P)
    n_seeds = {"user": B, "post": (1 + k) * B}
    model = make_model()
    ll = minibatch.LinkLoss(B, n_seeds["user"], n_seeds["post"], DEV, **lkw)
    step = minibatch.CapturedStep(model, g.x_dict, s, n_seeds, ll, None, slack=16)
    ls = minibatch.LinkSampler(step, ei, P, **skw)
    order = torch.randperm(int(ei.shape[1]), device=DEV,
                           generator=torch.Generator(device=DEV).manual_seed(7))

    def eager(b):
        lb = minibatch.link_batch(ei, order[b * B:(b + 1) * B], P,
                                  torch.Generator(device=DEV).manual_seed(40 + b), k, **skw)
        lb.mb = s.sample(lb.seeds, seed=b)
        return lb

    lb0 = eager(0)
    ll.load(lb0.pu, lb0.pp, lb0.pn, lb0.w, lb0.seeds["post"])
    step.capture(lb0.mb)
    logq = lkw["logq"]
    for b in (1, 2, 6):
        ls.prepare(order[b * B:(b + 1) * B], b, torch.Generator(device=DEV).manual_seed(40 + b))
        got_loss = float(step.step())
        got = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        again = float(step.step())                 # the same staged batch, replayed
        assert again == got_loss
        for n, p in model.named_parameters():
            assert torch.equal(p.grad, got[n]), n
        lb = eager(b)
        ref_model = make_model()
        ref_model.load_state_dict(model.state_dict())
        out = sampler.forward_blocks(ref_model, lb.mb, g.x_dict)
        ref = ops.link_loss(out["user"], out["post"], torch.stack([lb.pu, lb.pp]), lb.pn, lb.w,
                            weighting="edge", logq=logq[lb.seeds["post"]])
        ref.backward()
        want = float(ref.detach())
        print(f"batch {b}: captured {got_loss!r} torch {want!r} "
              f"rel {abs(got_loss - want) / abs(want):.3e}")
        assert abs(got_loss - want) <= 2e-6 * abs(want), (got_loss, want)
        for n, p in ref_model.named_parameters():
            _close(got[n], p.grad, n)


def test_n_total_scales_the_k_negative_loss():
    """``n_total`` = the positives of all ranks: a loss made with twice the batch's count gives
    half the value on the same staged batch (1/n_total per positive, 1/(n_total·k) per
    negative), so per-rank losses add up to the global batch's."""
    from truth_recommendation_gnn_amd import minibatch
    B, k, d = 48, 3, 16
    gen = torch.Generator(device=DEV).manual_seed(2)
    pu = torch.randint(0, B, (B,), device=DEV, generator=gen, dtype=torch.int32)
    pp = torch.randint(0, 4 * B, (B,), device=DEV, generator=gen, dtype=torch.int32)
    pn = torch.randint(0, 4 * B, (B, k), device=DEV, generator=gen, dtype=torch.int32)
    out = {"user": torch.randn(B, d, device=DEV, generator=gen) * 0.3,
           "post": torch.randn(4 * B, d, device=DEV, generator=gen) * 0.3}
    vals = []
    for n_total in (0, 2 * B):
        ll = minibatch.LinkLoss(B, B, 4 * B, DEV, n_total=n_total, num_neg=k)
        ll.load(pu, pp, pn)
        vals.append(float(ll(out)))
    ref = (torch.nn.functional.softplus(-(out["user"][pu.long()] * out["post"][pp.long()]).sum(1))
           .mean() + torch.nn.functional.softplus(
               (out["user"][pu.long()][:, None, :] * out["post"][pn.long()]).sum(-1)).mean())
    assert abs(vals[0] - float(ref)) <= 2e-6 * abs(float(ref))
    assert abs(vals[1] - 0.5 * vals[0]) <= 1e-6 * abs(vals[0])


def test_argument_errors():
    """Every mismatch is a ``ValueError`` raised before any launch."""
    from truth_recommendation_gnn_amd import minibatch
    g, s, make_model, ei, U, P, B = _link_setup()
    i32 = dict(dtype=torch.int32, device=DEV)
    pu, pp = torch.zeros(B, **i32), torch.zeros(B, **i32)
    logq = torch.zeros(P, device=DEV)
    ll = minibatch.LinkLoss(B, B, 4 * B, DEV, num_neg=3)
    for pn in (torch.zeros(B, **i32), torch.zeros(B, 2, **i32)):
        with pytest.raises(ValueError, match="pn"):
            ll.prepare(pu, pp, pn)
    pn3 = torch.zeros(B, 3, **i32)
    with pytest.raises(ValueError, match="w "):
        ll.prepare(pu, pp, pn3, torch.ones(B, device=DEV))           # w without "edge"
    with pytest.raises(ValueError, match="seeds_p"):
        ll.prepare(pu, pp, pn3, None, torch.zeros(4, **i32))         # seeds_p without logq
    with pytest.raises(ValueError, match="w "):
        minibatch.LinkLoss(B, B, 4 * B, DEV, num_neg=3, weighting="edge").prepare(pu, pp, pn3)
    with pytest.raises(ValueError, match="seeds_p"):
        minibatch.LinkLoss(B, B, 4 * B, DEV, num_neg=3, logq=logq).prepare(pu, pp, pn3)
    with pytest.raises(ValueError, match="pn"):
        minibatch.LinkLoss(B, B, 2 * B, DEV).prepare(pu, pp, pn3)    # the default takes k = 1
    for bad in (torch.zeros(P, 2, device=DEV), torch.zeros(P, dtype=torch.int64, device=DEV),
                torch.full((P,), float("inf"), device=DEV),
                torch.tensor([0.0, float("nan")], device=DEV)):
        with pytest.raises(ValueError, match="logq"):
            minibatch.LinkLoss(B, B, 4 * B, DEV, num_neg=3, logq=bad)
    with pytest.raises(ValueError, match="weighting"):
        minibatch.LinkLoss(B, B, 2 * B, DEV, weighting="sum")
    # LinkSampler: the post-seed capacity must be (1 + k) B; pos_weights one per edge
    model = make_model()
    n_seeds = {"user": B, "post": 2 * B}
    step = minibatch.CapturedStep(model, g.x_dict, s, n_seeds,
                                  minibatch.LinkLoss(B, B, 2 * B, DEV, num_neg=3), None, slack=16)
    with pytest.raises(ValueError, match="posts"):
        minibatch.LinkSampler(step, ei, P)
    n_seeds = {"user": B, "post": 3 * B}
    step = minibatch.CapturedStep(
        model, g.x_dict, s, n_seeds,
        minibatch.LinkLoss(B, B, 3 * B, DEV, num_neg=2, weighting="edge"), None, slack=16)
    for bad in (None, torch.ones(int(ei.shape[1]) - 1, device=DEV)):
        with pytest.raises(ValueError, match="pos_weights"):
            minibatch.LinkSampler(step, ei, P, pos_weights=bad)
    with pytest.raises(ValueError, match="pos_weights"):
        minibatch.link_batch(ei, torch.arange(B, device=DEV), P,
                             pos_weights=torch.ones(3, device=DEV))
    step = minibatch.CapturedStep(
        model, g.x_dict, s, n_seeds,
        minibatch.LinkLoss(B, B, 3 * B, DEV, num_neg=2, logq=torch.zeros(P + 1, device=DEV)),
        None, slack=16)
    with pytest.raises(ValueError, match="logq"):
        minibatch.LinkSampler(step, ei, P)


def test_default_layout_and_calls_are_unchanged():
    """With no option the arena holds the nine entries it held, at the same sizes; the optional
    entries come after them and only when asked for."""
    from truth_recommendation_gnn_amd import minibatch
    B = 48
    ll = minibatch.LinkLoss(B, B, 2 * B, DEV)
    assert list(ll.arena.layout) == list(_NINE)
    assert [ll.arena.layout[n][1] for n in _NINE] == [B + 1, B, B, B, 2 * B + 1, B, B,
                                                      2 * B + 1, B]
    full = minibatch.LinkLoss(B, B, 4 * B, DEV, num_neg=3, weighting="edge",
                              logq=torch.zeros(9, device=DEV))
    assert list(full.arena.layout) == list(_NINE) + ["w_user", "w_post", "logq"]
    assert full.arena.layout["neg"][1] == 3 * B and full.arena.layout["n_users"][1] == 3 * B
