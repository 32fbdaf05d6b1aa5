"""Static layer-1 aggregates (ops.gather_mean(static=True)): the mean of a model INPUT
table over a relation is computed once and kept on the RelationCSR, keyed by the live tensor
object, its pointer, shape, strides and version.  The kept values come from the very call a step
made before, so everything a training step produces must be bit-identical with the keeping off.

Graph: 300 users, 40 posts, 3,000 engages edges (+ the reverse relation), d = h = 128, two-layer
HeteroSAGE.  Post 0 has 280 distinct users — above the skew chunk (64) in one pass and in each of
3 source-block passes — so the heavy-row fixup runs."""
import gc

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import ops

gpu = pytest.mark.gpu
NU, NP, E, H = 300, 40, 3000, 128
ENG, REV = ("user", "engages", "post"), ("post", "rev_engages", "user")
RELS = [(ENG, 1.0), (REV, 1.0)]


@pytest.fixture(scope="module")
def graph():
    """Edges, fixed negatives and interaction weights on the device; never written."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(5)
    heavy = rng.permutation(NU)[:280]
    u = np.concatenate([heavy, rng.integers(0, NU, E - 280)])
    p = np.concatenate([np.zeros(280, np.int64), rng.integers(1, NP, E - 280)])
    ei = torch.from_numpy(np.stack([u, p]).astype(np.int64)).to(dev)
    edges = {ENG: ei, REV: ei.flip(0).contiguous()}
    neg = torch.from_numpy(rng.integers(0, NP, E).astype(np.int64)).to(dev)
    pw = torch.from_numpy((rng.random(E) + 0.5).astype(np.float32)).to(dev)
    return edges, neg, pw


def _inputs(d=H, requires_grad=False):
    gen = torch.Generator().manual_seed(11)
    x = {"user": torch.randn(NU, d, generator=gen).cuda(),
         "post": torch.randn(NP, d, generator=gen).cuda()}
    if requires_grad:
        for t in x.values():
            t.requires_grad_()
    return x


def _model(d=H):
    from truth_recommendation_gnn_amd import HeteroSAGE
    torch.manual_seed(3)
    return HeteroSAGE(H, RELS, num_layers=2, in_channels=d).cuda()


def _step(model, opt, x, graph):
    edges, neg, pw = graph
    opt.zero_grad(set_to_none=True)
    for t in x.values():
        t.grad = None
    out = model(x, edges)
    loss = ops.edge_bce_loss(out["user"], out["post"], edges[ENG], neg, pw)
    loss.backward()
    opt.step()
    rec = {"loss": loss.detach().clone(), "out.user": out["user"].detach().clone(),
           "out.post": out["post"].detach().clone()}
    for n, p in model.named_parameters():
        rec["grad." + n] = p.grad.detach().clone()
        rec["param." + n] = p.detach().clone()
    for t, v in x.items():
        if v.grad is not None:
            rec["xgrad." + t] = v.grad.detach().clone()
    return rec


def _train(monkeypatch, mode, graph, steps=3, d=H, requires_grad=False, between=None, x=None):
    """``steps`` training steps (forward, edge_bce_loss, backward, Adam) from seeded weights and
    inputs with HGNN_STATIC_AGG = ``mode``; ``between(x, step)`` runs after each step."""
    from truth_recommendation_gnn_amd import optim
    monkeypatch.setattr(ops, "STATIC_AGG", mode)
    ops.clear_static_aggregates()
    x = _inputs(d, requires_grad) if x is None else x
    model = _model(d)
    opt = optim.Adam(model.parameters(), lr=1e-2)
    recs = []
    for s in range(steps):
        recs.append(_step(model, opt, x, graph))
        if between is not None:
            between(x, s)
    return recs, x


def _assert_same(got, want):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w)
        for k in w:
            assert torch.equal(g[k], w[k]), (s, k)


class _blocked:
    """The user table (153,600 B) in 3 source-block passes, the post table in one; set and
    restored the way bench._one_pass_k1 does."""

    def __enter__(self):
        self.keep = (ops.GATHER_BLOCK_BYTES, ops.GATHER_BLOCK_SLICE)
        ops.GATHER_BLOCK_BYTES, ops.GATHER_BLOCK_SLICE = 100_000, 60_000
        assert ops.gather_blocks(torch.empty(NU, H, device="meta"), E) == 3
        assert ops.gather_blocks(torch.empty(NP, H, device="meta"), E) == 1

    def __exit__(self, *exc):
        ops.GATHER_BLOCK_BYTES, ops.GATHER_BLOCK_SLICE = self.keep


@gpu
@pytest.mark.parametrize("blocked", [False, True])
def test_three_steps_bitwise_equal_to_cache_off(monkeypatch, graph, blocked):
    import contextlib
    with (_blocked() if blocked else contextlib.nullcontext()):
        on, _ = _train(monkeypatch, "1", graph)
        assert ops.static_aggregate_count() == 2
        off, _ = _train(monkeypatch, "0", graph)
        assert ops.static_aggregate_count() == 0
    _assert_same(on, off)
    from truth_recommendation_gnn_amd.graph import relation_csr
    csr = relation_csr(graph[0][ENG], NU, NP)
    assert csr.fwd.plan.n_heavy >= 1          # the heavy-row fixup ran
    if blocked:
        assert all(p.plan.n_heavy >= 1 for p in csr.blocks("fwd", 3)[0])


@gpu
def test_layer1_gathers_launch_once_layer2_every_step(monkeypatch, graph):
    """Input width 64, hidden 128: the kernel names tell layer 1's gathers (x64) from layer 2's
    (x128; the post->user one gathers the pre-projected rows)."""
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        _train(monkeypatch, "1", graph, d=64)
    finally:
        ops.set_timer(None)
    n = {k: v["launches"] for k, v in timer.summary().items() if k.startswith("gather_fwd")}
    print(n)
    assert n == {f"gather_fwd[{NP}<-{NU}]x64": 1, f"gather_fwd[{NU}<-{NP}]x64": 1,
                 f"gather_fwd[{NP}<-{NU}]x128": 3, f"gather_fwd[{NU}<-{NP}]x128": 3}


@gpu
def test_in_place_mutation_recomputes(monkeypatch, graph):
    def double(x, s):
        if s == 0:
            for t in x.values():
                t.mul_(2)                     # bumps _version: the kept aggregates must miss
    on, _ = _train(monkeypatch, "1", graph, between=double)
    off, _ = _train(monkeypatch, "0", graph, between=double)
    _assert_same(on, off)
    assert not torch.equal(on[0]["out.user"], on[1]["out.user"])


@gpu
def test_dead_table_drops_its_entry_and_reused_storage_misses(monkeypatch, graph):
    edges = graph[0]
    monkeypatch.setattr(ops, "STATIC_AGG", "1")
    ops.clear_static_aggregates()
    model = _model()
    x = _inputs()
    out = model(x, edges)
    assert ops.static_aggregate_count() == 2
    ptrs = {t: v.data_ptr() for t, v in x.items()}
    del out, x
    gc.collect()
    assert ops.static_aggregate_count() == 0
    # same shapes, other values; the allocator may hand the freed blocks back
    y = {"user": torch.full((NU, H), 0.25, device="cuda"),
         "post": torch.full((NP, H), -0.5, device="cuda")}
    print("storage reused:", {t: v.data_ptr() == ptrs[t] for t, v in y.items()})
    got = {t: v.detach().clone() for t, v in model(y, edges).items()}
    assert ops.static_aggregate_count() == 2
    monkeypatch.setattr(ops, "STATIC_AGG", "0")
    want = model(y, edges)
    for t in want:
        assert torch.equal(got[t], want[t].detach()), t


@gpu
def test_inputs_that_need_a_gradient_are_never_kept(monkeypatch, graph):
    on, _ = _train(monkeypatch, "1", graph, requires_grad=True)
    assert ops.static_aggregate_count() == 0
    off, _ = _train(monkeypatch, "0", graph, requires_grad=True)
    assert "xgrad.user" in on[0] and "xgrad.post" in on[0]
    _assert_same(on, off)


@gpu
def test_sampled_steps_never_keep_an_aggregate(monkeypatch):
    """A sampled mini-batch step — eager over the blocks, and captured / replayed through
    minibatch.CapturedStep — leaves no entry: its block tables are refilled through raw pointers."""
    from truth_recommendation_gnn_amd import HeteroSAGE, minibatch, sampler, synth
    monkeypatch.setattr(ops, "STATIC_AGG", "1")
    ops.clear_static_aggregates()
    dev = torch.device("cuda")
    cfg = synth.dataclasses.replace(synth.scaled("cfg5", 0.0002), dim=16, hidden=16)
    g = synth.make_graph(cfg, device=dev)
    rels = [(synth.REV_ENGAGES, 1.0), (synth.SOCIAL, 0.75), (synth.ENGAGES, 1.0),
            (synth.POST_POST, 0.5)]
    num = {"user": cfg.num_users, "post": cfg.num_posts}
    s = sampler.NeighborSampler(num, g.edge_index_dict, [et for et, _ in rels], [5, 3])
    seeds = {t: torch.arange(24, device=dev) for t in num}
    torch.manual_seed(synth.WEIGHT_SEED)
    model = HeteroSAGE(cfg.hidden, rels, num_layers=2, in_channels=cfg.dim).to(dev)

    def loss_of(out):
        return (out["user"] * out["post"]).sum(1).sigmoid().mean()

    mb = s.sample(seeds, seed=0)
    loss_of(sampler.forward_blocks(model, mb, g.x_dict)).backward()
    assert ops.static_aggregate_count() == 0
    step = minibatch.CapturedStep(model, g.x_dict, s, {"user": 24, "post": 24}, loss_of, None,
                                  slack=16)
    step.capture(mb)
    step.step(s.sample(seeds, seed=1))
    torch.cuda.synchronize()
    assert ops.static_aggregate_count() == 0


@gpu
def test_entry_made_under_no_grad_serves_the_training_step(monkeypatch, graph):
    """bench.py's CSR-building call runs the model under no_grad first.  d = 64 < h keeps both
    layer-1 relations aggregate-first there, so both entries exist before the first step."""
    from truth_recommendation_gnn_amd import optim
    edges = graph[0]
    off, _ = _train(monkeypatch, "0", graph, steps=1, d=64)
    monkeypatch.setattr(ops, "STATIC_AGG", "1")
    ops.clear_static_aggregates()
    x, model = _inputs(64), _model(64)
    with torch.no_grad():
        model(x, edges)
    assert ops.static_aggregate_count() == 2
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        on = [_step(model, optim.Adam(model.parameters(), lr=1e-2), x, graph)]
    finally:
        ops.set_timer(None)
    names = [k for k in timer.summary() if k.startswith("gather_fwd")]
    assert sorted(names) == sorted([f"gather_fwd[{NP}<-{NU}]x128", f"gather_fwd[{NU}<-{NP}]x128"])
    _assert_same(on, off)


@gpu
def test_check_mode_raises_on_a_raw_pointer_write(monkeypatch, graph):
    """HGNN_STATIC_AGG=check: the project's own row gather writes into a view of the user table
    (a native kernel through a raw pointer: no version bump); the next forward raises and names
    the relation.  Without the write the same forwards pass."""
    from truth_recommendation_gnn_amd import _native as N
    edges = graph[0]
    monkeypatch.setattr(ops, "STATIC_AGG", "check")
    ops.clear_static_aggregates()
    model, x = _model(), _inputs()
    with torch.no_grad():
        first = model(x, edges)
    out = model(x, edges)                          # hits: fingerprints recomputed, silent
    loss = out["user"].sum() + out["post"].sum()
    loss.backward()
    with torch.no_grad():
        again = model(x, edges)
    for t in first:
        assert torch.equal(first[t], again[t])
    version = x["user"]._version
    src = torch.ones(16, H, device="cuda")
    ids = torch.arange(8, dtype=torch.int32, device="cuda")
    view = x["user"][:8]
    N.check(N.lib().hgnn_gather_rows_multi(1, N.ptr_array([src]), N.ptr_array([ids]),
                                           N.i64_array([8]), H, N.ptr_array([view]),
                                           N.stream_ptr(src.device)), "hgnn_gather_rows_multi")
    assert x["user"]._version == version and bool((x["user"][:8] == 1).all())
    with pytest.raises(ops.StaleAggregateError, match="user->post"):
        model(x, edges)
    ops.clear_static_aggregates()                  # what the writer is told to do
    got = model(x, edges)
    monkeypatch.setattr(ops, "STATIC_AGG", "0")
    want = model(x, edges)
    for t in want:
        assert torch.equal(got[t].detach(), want[t].detach())


# ----------------------------------------------------------------------------- no GPU
class _Rel:
    n_src, n_dst, num_edges = 5, 3, 7


def test_key_logic_with_an_injected_gather(monkeypatch):
    """Hit, version miss, other-object miss, blocking miss, flag off, clear, dead table, and the
    check mode's comparison — with a counting stand-in for the gather (no GPU)."""
    monkeypatch.setattr(ops, "STATIC_AGG", "1")
    ops.clear_static_aggregates()
    calls = []

    def compute():
        calls.append(1)
        return torch.full((3, 2), float(len(calls)))

    def get(t, rel, blocks=1, **kw):
        return ops._static_aggregate(t, rel, blocks, "user->post", compute, **kw)

    rel, x = _Rel(), torch.randn(5, 2)
    a = get(x, rel)
    assert get(x, rel) is a and len(calls) == 1 and ops.static_aggregate_count() == 1
    x.add_(1)                                            # version bump
    b = get(x, rel)
    assert b is not a and len(calls) == 2 and ops.static_aggregate_count() == 1
    assert get(x, rel) is b and len(calls) == 2
    v = x.view(5, 2)                                     # same pointer and version, other object
    assert v.data_ptr() == x.data_ptr() and v._version == x._version
    get(v, rel)
    assert len(calls) == 3
    get(x, rel)                                          # the entry was replaced by v's
    assert len(calls) == 4
    get(x, rel, blocks=3)                                # another blocking: other rounding
    assert len(calls) == 5
    other = _Rel()                                       # entries live on the relation
    get(x, other)
    assert len(calls) == 6 and ops.static_aggregate_count() == 2
    monkeypatch.setattr(ops, "STATIC_AGG", "0")          # off: computes, keeps nothing new
    get(x, other)
    get(x, other)
    assert len(calls) == 8
    monkeypatch.setattr(ops, "STATIC_AGG", "1")
    get(x, other)
    assert len(calls) == 8                               # (the entry from before is still valid)
    ops.clear_static_aggregates()
    assert ops.static_aggregate_count() == 0
    get(x, other)
    assert len(calls) == 9 and ops.static_aggregate_count() == 1
    del x, v
    gc.collect()                                         # the table died: its entry with it
    assert ops.static_aggregate_count() == 0
    y = torch.randn(5, 2)
    get(y, other)
    assert len(calls) == 10
    del rel, other                                       # entries die with the relation
    gc.collect()
    assert ops.static_aggregate_count() == 0
    # check mode: the stored fingerprint is compared on every hit
    monkeypatch.setattr(ops, "STATIC_AGG", "check")
    state = {"fp": 17, "n": 0}

    def fingerprint(t):
        state["n"] += 1
        return state["fp"]

    rel = _Rel()
    c = get(y, rel, fingerprint=fingerprint)
    assert get(y, rel, fingerprint=fingerprint) is c and state["n"] == 2 and len(calls) == 11
    state["fp"] = 18                                     # memory changed, version did not
    with pytest.raises(ops.StaleAggregateError, match="user->post"):
        get(y, rel, fingerprint=fingerprint)
    ops.clear_static_aggregates()
    assert get(y, rel, fingerprint=fingerprint) is not c and len(calls) == 12


def test_static_is_refused_for_accumulating_gathers_and_sampled_blocks():
    x = torch.zeros(5, 4)
    with pytest.raises(ValueError, match="never accumulated"):
        ops.gather_mean(x, _Rel(), out=torch.zeros(3, 4), static=True)
    g = ops.DstGroup("post", (("user", _Rel()),), True, True, (), n_root=2, static=(True,))
    with pytest.raises(ValueError, match="never static"):
        ops.hetero_layer(ops.LayerSpec(("post", "user"), (g,)),
                         {"user": torch.zeros(5, 4, device="meta"),
                          "post": torch.zeros(3, 4, device="meta")}, [])


def test_only_first_layer_inputs_are_flagged(monkeypatch):
    """nn.HeteroSAGE flags layer 1's aggregate-first relations over inputs without a gradient
    and nothing else — also under no_grad, where every intermediate has requires_grad False."""
    from truth_recommendation_gnn_amd import HeteroSAGE, nn
    specs = []

    def fake_layer(spec, h, weights):
        specs.append(spec)
        return {g.dst: torch.zeros(h[g.dst].shape[0], 8) for g in spec.groups}

    class _Csr:
        pass

    monkeypatch.setattr(nn.ops, "hetero_layer", fake_layer)
    monkeypatch.setattr(nn, "relation_csr", lambda ei, ns, nd: _Csr())
    monkeypatch.setattr(nn, "_fused_weights_layer", lambda convs, msgs, h: None)
    model = HeteroSAGE(8, RELS, num_layers=3, in_channels=8)
    edges = {ENG: torch.zeros(2, 4, dtype=torch.long), REV: torch.zeros(2, 4, dtype=torch.long)}
    x = {"user": torch.randn(30, 8), "post": torch.randn(4, 8)}
    for ctx in (torch.enable_grad(), torch.no_grad()):
        specs.clear()
        with ctx:
            model(x, edges)
        for li, spec in enumerate(specs):
            for g in spec.groups:
                want = tuple(li == 0 and not p for p in g.pre)
                assert tuple(g.static) == want, (li, g.dst)
        assert any(any(g.static) for g in specs[0].groups)
    specs.clear()
    model({t: v.clone().requires_grad_() for t, v in x.items()}, edges)
    assert not any(any(g.static) for spec in specs for g in spec.groups)
