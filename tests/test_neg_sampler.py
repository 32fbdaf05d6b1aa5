"""Popularity-weighted negatives: the device sampler (``ops.PostDistribution``,
``ops.sample_negatives(distribution=, avoid=)``) and the dP gather with a per-step plan of the
negatives' lists (``ops.SkewedNegatives`` -> ``hgnn_score_gather2_planned``).

Reference mapping of a draw, restated here with Python integers:

    x = splitmix64(seed + c * golden)        (``synth._hash64``'s mixer, as hgnn_uniform_i32's)
    r = (x * T) >> 64                        (the high half of the 128-bit product)
    j = bisect_right(cdf[1:], r)             (the unique post with cdf[j] <= r < cdf[j + 1])

The draws are compared elementwise and exactly.  The loss and its gradients are compared with the
float64 restatement of ``tests/test_loss_multi_neg.py`` (copied: ``_graph``, ``_tables``,
``_ref64``) at that file's tolerance, rtol 1e-4 and atol 1e-5 of the reference's largest entry;
for bf16 rows the restatement reads the tables rounded to bf16, the numbers both kernels read."""
import ctypes
import types
from bisect import bisect_right

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import _native as N
from truth_recommendation_gnn_amd import metrics, ops

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
HGNN_E_ARG = 1001
BCE = torch.nn.functional.binary_cross_entropy_with_logits


# ----------------------------------------------------------------------------- reference
def splitmix64(seed: int, c: int) -> int:
    x = (seed + c * GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def cdf_of(q):
    cdf = [0]
    for v in q:
        cdf.append(cdf[-1] + int(v))
    return cdf


def ref_draw(seed: int, c: int, cdf) -> int:
    r = (splitmix64(seed, c) * cdf[-1]) >> 64
    return bisect_right(cdf, r, 1) - 1


def ref_uniform(seed: int, c: int, hi: int) -> int:
    return ((splitmix64(seed, c) >> 32) * hi) >> 32


def ref_draws(seed: int, n: int, cdf):
    tail = cdf[1:]
    T = cdf[-1]
    return np.array([bisect_right(tail, (splitmix64(seed, c) * T) >> 64) for c in range(n)],
                    dtype=np.int64)


def ref_avoid(seed, n, k, cdf, n_posts, uop, seen, tries):
    """The rejection loop: (draws, how many kept a seen post)."""
    out, kept = np.empty(n, dtype=np.int64), 0
    for i in range(n):
        s = seen[int(uop[i // k])]
        for t in range(tries):
            c = i + t * n
            post = ref_draw(seed, c, cdf) if cdf is not None else ref_uniform(seed, c, n_posts)
            if post not in s:
                break
        else:
            kept += 1
        out[i] = post
    return out, kept


def zipf_q(n_posts: int, zero=()):
    """Integer Zipf(1) weights, top weight 2^20, with the posts of ``zero`` set to 0."""
    q = np.maximum((1 << 20) // np.arange(1, n_posts + 1), 1).astype(np.int64)
    for lo, hi in zero:
        q[lo:hi] = 0
    return q


# ----------------------------------------------------------------------------- CPU
def test_reference_mapping_samples_the_distribution():
    n_posts, n, seed = 50, 200_000, 0x1234567890ABCDEF
    w = 1.0 / np.arange(1, n_posts + 1)
    w[[0, 7, 49]] = 0.0
    q = np.floor(w / w.max() * (2**32 - 1)).astype(np.int64)
    cdf = cdf_of(q)
    counts = np.bincount(ref_draws(seed, n, cdf), minlength=n_posts)
    p = q / q.sum()
    assert counts[[0, 7, 49]].sum() == 0
    z = (counts - n * p)[q > 0] / np.sqrt(n * p * (1 - p))[q > 0]
    print("max |z| =", float(np.abs(z).max()))
    assert np.abs(z).max() <= 6.0
    # the scalar restatement is the vectorised one
    assert [ref_draw(seed, c, cdf) for c in range(200)] == list(ref_draws(seed, 200, cdf))


def test_argument_errors_that_need_no_device():
    with pytest.raises(ValueError, match="weights must be >= 0"):
        ops.PostDistribution(torch.tensor([1.0, -0.5, 2.0]))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weights must be finite"):
            ops.PostDistribution(torch.tensor([1.0, bad, 2.0]))
    with pytest.raises(ValueError, match="all zero"):
        ops.PostDistribution(torch.zeros(4))
    with pytest.raises(ValueError, match="all zero"):
        ops.PostDistribution(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"integer weights must lie in \[0, 2\^32\)"):
        ops.PostDistribution(torch.tensor([1, 2**32, 3]))
    with pytest.raises(ValueError, match=r"integer weights must lie in \[0, 2\^32\)"):
        ops.PostDistribution(torch.tensor([1, -1, 3]))
    with pytest.raises(ValueError, match=r"\[num_posts\]"):
        ops.PostDistribution(torch.ones(2, 2))
    ei = torch.tensor([[0, 1, 2], [1, 0, 1]])
    marker = object()     # refused before it is looked at
    with pytest.raises(ValueError, match="draw_negatives: distribution / avoid"):
        ops.draw_negatives(ei, 3, distribution=marker)
    with pytest.raises(ValueError, match="draw_negatives: distribution / avoid"):
        ops.draw_negatives(ei, 3, avoid=marker)
    # SkewedNegatives: int32 [E] / [E, k] only, the user order only, never the sharded step
    with pytest.raises(ValueError, match="int32 tensor"):
        ops.SkewedNegatives(torch.zeros(3, dtype=torch.int64))
    sk = ops.SkewedNegatives(torch.zeros(3, dtype=torch.int32))
    assert sk.shape == (3,) and sk.dtype == torch.int32 and sk.values.dtype == torch.int32
    assert ops.SkewedNegatives(torch.zeros(3, 2, dtype=torch.int32)).shape == (3, 2)
    U, P, w, one = torch.randn(3, 8), torch.randn(2, 8), torch.ones(3), torch.ones(())
    with pytest.raises(ValueError, match="SkewedNegatives do not combine with ready"):
        ops.edge_bce_loss(U, P, ei, sk, w, neg_order="user", ready=lambda: None)
    for kw in ({"ready": lambda: None}, {"on_dP": lambda dP: None}, {"p_chunks": [(0, 2, None)]}):
        with pytest.raises(ValueError, match="SkewedNegatives do not combine with "
                           + next(iter(kw))):
            ops.edge_bce_loss_raw(U, P, ei, sk, 3, one, neg_order="user", **kw)
    with pytest.raises(ValueError, match="user-grouped order"):
        ops.edge_bce_loss(U, P, ei, sk, w, neg_order="edge")
    with pytest.raises(TypeError, match="SkewedNegatives.values"):
        ops.link_loss(U, P, ei, sk, w)
    # a presort of one kind is refused by a loss over the other
    plain = ops.PresortedNegatives(None, sk.values, "user", 2, None, None, 1)
    assert not plain.planned
    with pytest.raises(ValueError, match="grouped without a plan"):
        plain.check_draws(sk, "user", "edge_bce_loss")
    planned = ops.PresortedNegatives(None, sk, "user", 2, None, None, 1, plan=object())
    assert planned.planned
    with pytest.raises(ValueError, match="grouped with a plan"):
        planned.check_draws(sk.values, "user", "edge_bce_loss")
    planned.check_draws(sk, "user", "edge_bce_loss")


def test_c_entries_check_their_arguments_before_any_launch():
    lib = N.lib()
    buf = (ctypes.c_int64 * 4)()
    x = ctypes.c_void_p(ctypes.addressof(buf))     # non-null, never dereferenced

    def err():
        return lib.hgnn_last_error_string()

    def draw(seed=x, n=5, cdf=x, n_posts=9, T=100, guide=x, shift=0, n_guide=128, out=x):
        return lib.hgnn_weighted_i32(seed, n, cdf, n_posts, T, guide, shift, n_guide, out, None)

    assert draw(n=-1) == HGNN_E_ARG and b"n=-1" in err()
    assert draw(T=0) == HGNN_E_ARG and b"T=0" in err()
    assert draw(cdf=None) == HGNN_E_ARG and b"null cdf" in err()
    assert draw(guide=None) == HGNN_E_ARG and b"null guide" in err()
    assert draw(seed=None) == HGNN_E_ARG and b"null pointer" in err()
    assert draw(out=None) == HGNN_E_ARG and b"null pointer" in err()
    assert draw(n_posts=0) == HGNN_E_ARG and b"n_posts=0" in err()
    assert draw(T=1 << 40, n_guide=16) == HGNN_E_ARG and b"does not cover" in err()

    def avoid(n=6, k=3, cdf=x, T=100, tries=4, uop=x, rp=x, col=x, out=x, seed=x):
        return lib.hgnn_weighted_avoid_i32(seed, n, k, cdf, 9, T, x, 0, 128, uop, 4, rp, col,
                                           tries, out, None, None)

    assert avoid(n=-3) == HGNN_E_ARG and b"n=-3" in err()
    assert avoid(n=7) == HGNN_E_ARG and b"n=7 n_neg=3" in err()
    assert avoid(tries=0) == HGNN_E_ARG and b"tries=0" in err()
    assert avoid(T=0) == HGNN_E_ARG and b"T=0" in err()
    for kw in ({"uop": None}, {"rp": None}, {"col": None}, {"out": None}, {"seed": None}):
        assert avoid(**kw) == HGNN_E_ARG and b"null pointer" in err()
    assert lib.hgnn_weighted_cdf_build(None, 4, x, None, 0, None) == HGNN_E_ARG
    assert lib.hgnn_weighted_cdf_build(x, 0, x, None, 0, None) == HGNN_E_ARG
    assert lib.hgnn_weighted_cdf_build(x, 1 << 20, x, None, 0, None) == 1003      # workspace
    assert lib.hgnn_weighted_guide_build(x, 9, 0, 0, 16, x, None) == HGNN_E_ARG and b"T=0" in err()
    assert lib.hgnn_weighted_guide_build(None, 9, 10, 0, 16, x, None) == HGNN_E_ARG
    assert lib.hgnn_plan_device(x, 4, 64, 3, None, x, x, x, 1 << 20, None) == HGNN_E_ARG
    assert lib.hgnn_plan_device(x, 4, 64, -1, x, x, x, x, 1 << 20, None) == HGNN_E_ARG

    def planned(rows=0, d=64, rowptr_n=x, counts=x, out=x):
        return lib.hgnn_score_gather2_planned(rows, x, 4, x, d, x, x, None, rowptr_n, x, 4, x,
                                              0.5, None, None, 0, 0, 64, None, x, x, counts, 8,
                                              x, out, None)

    assert planned(rows=3) == HGNN_E_ARG and b"rows=3" in err()
    assert planned(d=0) == HGNN_E_ARG and b"bad sizes" in err()
    assert planned(rowptr_n=None) == HGNN_E_ARG and b"null rowptr" in err()
    assert planned(out=None) == HGNN_E_ARG
    assert planned(counts=None) == HGNN_E_ARG and b"null arrays" in err()
    assert planned(rows=1, d=12) == 1004 and b"bf16 rows need" in err()
    assert planned(rows=2, d=32) == 1004 and b"zero-packed" in err()


# ----------------------------------------------------------------------------- GPU: the draws
DEV = "cuda:0"
SEED = 0x1234567890ABCDEF & ((1 << 62) - 1)
NS = (1, 255, 256, 257, 100003)


def _seed_tensor(seed=SEED):
    return torch.tensor([seed], dtype=torch.int64, device=DEV)


def _device_draws(dist, n, seed=SEED):
    out = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    N.check(N.lib().hgnn_weighted_i32(N.ptr(_seed_tensor(seed)), n, *dist._table_args(),
                                      N.ptr(out), N.stream_ptr(out.device)), "hgnn_weighted_i32")
    return out.cpu().numpy().astype(np.int64)


def _weight_cases():
    cases = {"one_post": np.array([7], dtype=np.int64),
             "two_posts": np.array([1, 3], dtype=np.int64),
             "two_posts_first_zero": np.array([0, 5], dtype=np.int64),
             "five": np.array([0, 9, 0, 4, 0], dtype=np.int64),
             "zipf_1000": zipf_q(1000, [(0, 17), (400, 650), (990, 1000)]),
             "zipf_70001": zipf_q(70001, [(0, 3), (30000, 50000), (69000, 70001)]),
             "single_nonzero": np.zeros(1000, dtype=np.int64),
             "max_weights": np.full(3000, 2**32 - 1, dtype=np.int64),
             "one_max_then_ones": np.concatenate([[2**32 - 1], np.ones(1000)]).astype(np.int64)}
    cases["single_nonzero"][613] = 12345
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_weight_cases()))
def test_weighted_draws_equal_the_reference_mapping(case):
    q = _weight_cases()[case]
    dist = ops.PostDistribution(torch.from_numpy(q).to(DEV))
    cdf = cdf_of(q)
    assert dist.T == cdf[-1] and dist.num_posts == len(q)
    assert dist.cdf.dtype == torch.int64
    assert np.array_equal(dist.cdf.cpu().numpy(), np.concatenate([[0], np.cumsum(q)]))
    if case == "max_weights":
        assert dist.T.bit_length() == 44
    assert ((dist.T - 1) >> dist.shift) < dist.n_guide
    want = ref_draws(SEED, max(NS), cdf)
    assert (q[want] > 0).all()
    for n in NS:
        got = _device_draws(dist, n)
        assert np.array_equal(got, want[:n]), (case, n)
    # another seed: the draws move, the mapping holds
    other = 0x0FEDCBA987654321
    assert np.array_equal(_device_draws(dist, 257, other), ref_draws(other, 257, cdf))


@pytest.mark.gpu
def test_cdf_of_a_table_of_several_scan_tiles_and_float_quantisation():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 2**32, 70001).astype(np.int64)      # 35 tiles of the 64-bit scan
    dist = ops.PostDistribution(torch.from_numpy(q).to(DEV))
    assert np.array_equal(dist.cdf.cpu().numpy(), np.concatenate([[0], np.cumsum(q)]))
    w = torch.tensor([0.0, 1.0, 0.25, 2.0**-33, 1e-3], dtype=torch.float32)
    dist = ops.PostDistribution(w.to(DEV))
    want = np.floor(w.double().numpy() / 1.0 * (2**32 - 1)).astype(np.int64)
    assert want[3] == 0 and want[1] == 2**32 - 1             # below max * 2^-32: never drawn
    assert np.array_equal(dist.q.cpu().numpy(), want)
    ei = torch.tensor([[0, 1, 2, 3, 4, 5], [1, 1, 1, 3, 3, 4]], device=DEV)
    deg = ops.PostDistribution.from_degree(ei, 6)
    wd = np.array([0, 3, 0, 2, 1, 0], dtype=np.float64) ** 0.75
    assert np.array_equal(deg.q.cpu().numpy(), np.floor(wd / wd.max() * (2**32 - 1)).astype(np.int64))


def _small_graph():
    """200 users, 50 posts; user u has seen min(u // 3, 50) posts (0 to 50), chosen at random;
    user 199 is given every positive-weight post."""
    rng = np.random.default_rng(11)
    n_users, n_posts = 200, 50
    q = zipf_q(n_posts, [(0, 2), (20, 25)])
    seen = [set(rng.choice(n_posts, min(u // 3, n_posts), replace=False).tolist())
            for u in range(n_users)]
    seen[199] = set(np.nonzero(q)[0].tolist())
    su = np.concatenate([np.full(len(s), u) for u, s in enumerate(seen)]).astype(np.int64)
    sp = np.concatenate([np.array(sorted(s), dtype=np.int64) for s in seen])
    user = rng.integers(0, n_users, 700)
    user[:5] = 199
    post = rng.integers(0, n_posts, 700)
    return n_users, n_posts, q, seen, np.stack([su, sp]), np.stack([user, post])


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 3))
def test_rejection_equals_the_reference_loop(k):
    n_users, n_posts, q, seen, seen_e, pos = _small_graph()
    assert {len(s) for s in seen} >= {0, 50}
    ei = torch.from_numpy(pos).to(DEV)
    index = metrics.SeenIndex(torch.from_numpy(seen_e).to(DEV), n_users, n_posts)
    dist = ops.PostDistribution(torch.from_numpy(q).to(DEV))
    csr = ops.relation_csr_for_loss(ei, n_users, n_posts)
    uop = ops._user_of_pos(csr).cpu().numpy()
    E, cdf = pos.shape[1], cdf_of(q)
    n = E * k
    lib, s = N.lib(), N.stream_ptr(torch.device(DEV))
    plain = _device_draws(dist, n)
    uni = torch.empty(n, dtype=torch.int32, device=DEV)
    N.check(lib.hgnn_uniform_i32(N.ptr(_seed_tensor()), n, n_posts, N.ptr(uni), s), "uniform")
    uni = uni.cpu().numpy()
    for tries in (1, 4):
        for table, ref_cdf in ((dist._table_args(), cdf), ((None, n_posts, 0, None, 0, 0), None)):
            out = torch.full((n,), -1, dtype=torch.int32, device=DEV)
            kept = torch.tensor([5], dtype=torch.int64, device=DEV)      # incremented, not set
            N.check(lib.hgnn_weighted_avoid_i32(
                N.ptr(_seed_tensor()), n, k, *table, N.ptr(ops._user_of_pos(csr)), n_users,
                N.ptr(index.rowptr), N.ptr(index._col), tries, N.ptr(out), N.ptr(kept), s),
                "hgnn_weighted_avoid_i32")
            want, want_kept = ref_avoid(SEED, n, k, ref_cdf, n_posts, uop, seen, tries)
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (k, tries, ref_cdf is None)
            assert int(kept) == 5 + want_kept
            first = plain if ref_cdf is not None else uni
            unseen0 = np.array([first[i] not in seen[uop[i // k]] for i in range(n)])
            assert unseen0.any() and not unseen0.all()
            assert np.array_equal(got[unseen0], first[unseen0])          # attempt 0 is the plain draw
            if tries == 1:
                assert np.array_equal(got, first)
            if ref_cdf is not None:
                # the user who has seen every post that can be drawn keeps attempt tries - 1
                full = np.nonzero(uop == 199)[0]
                assert len(full) >= 5
                for p in full:
                    for j in range(k):
                        i = int(p) * k + j
                        assert got[i] == ref_draw(SEED, i + (tries - 1) * n, cdf)
                assert want_kept >= len(full) * k
    # the Python surface: the same draws from the generator's seed, the counter on the device
    gen = torch.Generator(DEV).manual_seed(77)
    seed = int(torch.randint(0, 2**62, (1,), device=DEV, dtype=torch.int64, generator=gen))
    kept = torch.zeros(1, dtype=torch.int64, device=DEV)
    sk = ops.sample_negatives(ei, n_posts, gen.manual_seed(77), num_neg=k, distribution=dist,
                              avoid=index, max_tries=4, kept_seen=kept)
    assert isinstance(sk, ops.SkewedNegatives) and sk.dtype == torch.int32
    assert tuple(sk.shape) == ((E,) if k == 1 else (E, k))
    want, want_kept = ref_avoid(seed, n, k, cdf, n_posts, uop, seen, 4)
    assert np.array_equal(sk.values.cpu().numpy().reshape(-1), want) and int(kept) == want_kept
    only = ops.sample_negatives(ei, n_posts, gen.manual_seed(77), num_neg=k, avoid=index)
    want, _ = ref_avoid(seed, n, k, None, n_posts, uop, seen, 4)
    assert np.array_equal(only.values.cpu().numpy().reshape(-1), want)


@pytest.mark.gpu
def test_sample_negatives_shapes_and_the_unchanged_default():
    n_users, n_posts, q, _, _, pos = _small_graph()
    ei = torch.from_numpy(pos).to(DEV)
    E = pos.shape[1]
    dist = ops.PostDistribution(torch.from_numpy(q).to(DEV))
    gen = torch.Generator(DEV)
    seed_t = torch.randint(0, 2**62, (1,), device=DEV, dtype=torch.int64,
                           generator=gen.manual_seed(3))
    seed = int(seed_t)
    three = ops.sample_negatives(ei, n_posts, gen.manual_seed(3), num_neg=3, distribution=dist)
    assert isinstance(three, ops.SkewedNegatives)
    assert tuple(three.shape) == (E, 3) and three.dtype == torch.int32
    want = ref_draws(seed, 3 * E, cdf_of(q)).reshape(E, 3)       # draw p * 3 + j at [p, j]
    assert np.array_equal(three.values.cpu().numpy(), want)
    one = ops.sample_negatives(ei, n_posts, gen.manual_seed(3), distribution=dist)
    assert tuple(one.shape) == (E,)
    assert np.array_equal(one.values.cpu().numpy(), ref_draws(seed, E, cdf_of(q)))
    # without the new arguments: the tensor hgnn_uniform_i32 gives for the generator's seed
    for k in (1, 3):
        plain = ops.sample_negatives(ei, n_posts, gen.manual_seed(3), num_neg=k)
        assert isinstance(plain, torch.Tensor) and plain.dtype == torch.int32
        ref = torch.empty(E * k, dtype=torch.int32, device=DEV)
        N.check(N.lib().hgnn_uniform_i32(N.ptr(seed_t), E * k, n_posts, N.ptr(ref),
                                         N.stream_ptr(ref.device)), "hgnn_uniform_i32")
        assert torch.equal(plain.reshape(-1), ref)
        assert tuple(plain.shape) == ((E,) if k == 1 else (E, k))
    with pytest.raises(ValueError, match="distribution is over 50 posts"):
        ops.sample_negatives(ei, n_posts + 1, distribution=dist)
    with pytest.raises(ValueError, match="max_tries=0"):
        ops.sample_negatives(ei, n_posts, distribution=dist, max_tries=0)


# ----------------------------------------------------------------------------- GPU: the gather
N_USERS, N_POSTS = 300, 37
BIG_USER, NO_EDGE_USER = 0, 1
NO_POS, HEAVY = 0, 1                        # posts: no positives / 200 positives
CHUNK = 64
UP = 2.5
RTOL, ATOL_SCALE = 1e-4, 1e-5


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


def _ref64(U, P, ei, neg, w, weighting):
    Ur, Pr = U.double().requires_grad_(), P.double().requires_grad_()
    u = Ur[ei[0]]
    sp = (u * Pr[ei[1]]).sum(1)
    sn = (u[:, None, :] * Pr[neg]).sum(-1) if neg.dim() == 2 else (u * Pr[neg]).sum(1)
    neg_loss = BCE(sn, torch.zeros_like(sn))
    if weighting == "edge":
        loss = (w.double() * BCE(sp, torch.ones_like(sp), reduction="none")).mean() + neg_loss
    else:
        loss = (w.double() * BCE(sp, torch.ones_like(sp))).mean() + neg_loss
    (loss * UP).backward()
    return loss.detach(), Ur.grad, Pr.grad


@pytest.fixture(scope="module")
def g():
    user, post = _graph()
    dev = torch.device(DEV)
    ei = torch.from_numpy(np.stack([user, post]))
    ei_d = ei.to(dev)
    E = int(ei.shape[1])
    csr = ops.relation_csr_for_loss(ei_d, N_USERS, N_POSTS)
    assert csr.fwd.plan.chunk == CHUNK and csr.fwd.plan.n_heavy > 0
    perm_u = csr.bwd.perm.cpu().long()
    deg = np.bincount(post, minlength=N_POSTS)
    # 0.9 of the mass on the post with 200 positives, 0.05 on the post without positives, none
    # on one post with more than a chunk of positives, the rest spread thin
    pos_only = int(np.nonzero((deg > CHUNK) & (np.arange(N_POSTS) > HEAVY))[0][0])
    w = np.full(N_POSTS, 0.05 / (N_POSTS - 3))
    w[HEAVY], w[NO_POS], w[pos_only] = 0.9, 0.05, 0.0
    dist = ops.PostDistribution(torch.from_numpy(w).to(dev))
    cdf = cdf_of(dist.q.cpu().numpy())
    negs = {}
    for k in (1, 3):
        assert E * k >= 2000
        gen = torch.Generator(dev)
        seed = int(torch.randint(0, 2**62, (1,), device=dev, dtype=torch.int64,
                                 generator=gen.manual_seed(40 + k)))
        sk = ops.sample_negatives(ei_d, N_POSTS, gen.manual_seed(40 + k), num_neg=k,
                                  distribution=dist)
        # the reference mapping alone gives the four cases
        ref = ref_draws(seed, E * k, cdf)
        cnt = np.bincount(ref, minlength=N_POSTS)
        assert np.array_equal(sk.values.cpu().numpy().reshape(-1), ref)
        assert deg[HEAVY] > CHUNK and cnt[HEAVY] > CHUNK              # heavy in both
        assert deg[NO_POS] == 0 and cnt[NO_POS] > CHUNK               # heavy negatives only
        assert deg[pos_only] > CHUNK and cnt[pos_only] == 0           # heavy positives only
        light = (deg <= CHUNK) & (cnt <= CHUNK) & (deg > 0) & (cnt > 0)
        assert light.any()                                            # neither
        assert (cnt > CHUNK).sum() == 2
        shape = (E,) if k == 1 else (E, k)
        neg_edge = torch.empty(shape, dtype=torch.int64)
        neg_edge[perm_u] = sk.values.cpu().long()                     # COO order, for the reference
        negs[k] = (sk, neg_edge)
    return types.SimpleNamespace(dev=dev, ei=ei, ei_d=ei_d, csr=csr, E=E, negs=negs,
                                 pos_only=pos_only)


_IN = {}


def _inputs(g, d, rows):
    """Tables, weights and the float64 references of one width and row format: built once."""
    key = (d, rows)
    if key not in _IN:
        U, P = _tables(d, relu=rows == "zp")
        w = torch.where(torch.arange(g.E) % 3 == 0, 3.0, 1.0)
        Ud, Pd = U.to(g.dev), P.to(g.dev)
        if rows == "bf16":      # the reference reads the numbers the kernels read
            U, P = ops.rows_to_bf16(Ud).float().cpu(), ops.rows_to_bf16(Pd).float().cpu()
        _IN[key] = types.SimpleNamespace(U=U, P=P, w=w, Ud=Ud, Pd=Pd, wd=w.to(g.dev), ref={})
    return _IN[key]


def _ref(g, t, k, weighting):
    if (k, weighting) not in t.ref:
        t.ref[(k, weighting)] = _ref64(t.U, t.P, g.ei, g.negs[k][1], t.w, weighting)
    return t.ref[(k, weighting)]


def _run(g, t, neg, rows, **kw):
    U, P = t.Ud.clone().requires_grad_(), t.Pd.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, g.ei_d, neg, t.wd, neg_order="user",
                             row_dtype="bf16" if rows == "bf16" else "fp32", **kw)
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
@pytest.mark.parametrize("rows", ("fp32", "bf16", "zp"))
@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("d", (64, 128))
def test_planned_gather_matches_float64(g, d, k, rows, monkeypatch):
    monkeypatch.setenv("HGNN_ZPACK", "1" if rows == "zp" else "0")
    t = _inputs(g, d, rows)
    sk = g.negs[k][0]
    for weighting in ("mean", "edge"):
        ref = _ref(g, t, k, weighting)
        got, names = _timed_names(lambda: _run(g, t, sk, rows, weighting=weighting))
        assert f"score_gather_planned[{N_POSTS}<-{N_USERS}]x{d}" in names
        assert "plan_negatives" in names
        assert (f"zpack[{N_USERS}]x{d}" in names) == (rows == "zp")
        for a, b, name in zip(got, ref, ("loss", "dU", "dP")):
            print(d, k, rows, weighting, name, float((a.double().cpu() - b).abs().max()),
                  float(b.abs().max()))
            close(a, b)
        for p in (HEAVY, NO_POS, g.pos_only):
            assert float(got[2][p].abs().max()) > 0
        again = _run(g, t, sk, rows, weighting=weighting)
        for a, b, name in zip(again, got, ("loss", "dU", "dP")):
            assert torch.equal(a, b), name
        # the same negatives as a plain tensor: the unplanned gather, the same numbers
        plain, names = _timed_names(lambda: _run(g, t, sk.values, rows, weighting=weighting))
        assert f"score_gather[{N_POSTS}<-{N_USERS}]x{d}" in names
        assert "plan_negatives" not in names
        for a, b in zip(plain, ref):
            close(a, b)
        for a, b in zip(plain, got):
            close(a, b)


@pytest.mark.gpu
def test_planned_gather_at_an_odd_width_and_a_list_of_exactly_one_chunk(g):
    """d = 200 (two float4 per lane) and d = 5 (scalar rows), and negatives built by hand: one
    post with exactly CHUNK negatives (light: the row's wave sums it), one with CHUNK + 1 (two
    chunks, the second of one entry) and one with 3 * CHUNK (whole chunks only)."""
    E = g.E
    neg = np.full(E, 5, dtype=np.int32)
    neg[:CHUNK] = 7
    neg[CHUNK:2 * CHUNK + 1] = 9
    neg[3 * CHUNK:6 * CHUNK] = 11
    rng = np.random.default_rng(3)
    neg = neg[rng.permutation(E)]
    sk = ops.SkewedNegatives(torch.from_numpy(neg).to(g.dev))
    neg_edge = torch.empty(E, dtype=torch.int64)
    neg_edge[g.csr.bwd.perm.cpu().long()] = torch.from_numpy(neg).long()
    for d in (200, 5):
        t = _inputs(g, d, "fp32")
        ref = _ref64(t.U, t.P, g.ei, neg_edge, t.w, "edge")
        got = _run(g, t, sk, "fp32", weighting="edge")
        for a, b in zip(got, ref):
            close(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 3))
def test_presorted_skewed_negatives_round_trip(g, k):
    t = _inputs(g, 64, "fp32")
    sk = g.negs[k][0]
    pre = ops.presort_negatives(N_USERS, N_POSTS, g.ei_d, sk, "user")
    assert pre.planned and pre.k == k and int(pre.rowptr[-1]) == k * g.E
    n_heavy, n_chunks = pre.plan.counts.tolist()
    lens = (pre.rowptr[1:] - pre.rowptr[:-1]).cpu().numpy()
    assert n_heavy == 2 and n_chunks == int(np.ceil(lens[lens > CHUNK] / CHUNK).sum())
    assert pre.plan.heavy_rows[:2].tolist() == [NO_POS, HEAVY]
    want = _run(g, t, sk, "fp32", weighting="edge")
    got = _run(g, t, sk, "fp32", weighting="edge", presorted=pre)
    for a, b, name in zip(got, want, ("loss", "dU", "dP")):
        assert torch.equal(a, b), name
    # refused by a plain call, and a plain presort by a planned call
    with pytest.raises(ValueError, match="grouped with a plan"):
        _run(g, t, sk.values, "fp32", presorted=pre)
    plain = ops.presort_negatives(N_USERS, N_POSTS, g.ei_d, sk.values, "user")
    assert not plain.planned
    with pytest.raises(ValueError, match="grouped without a plan"):
        _run(g, t, sk, "fp32", presorted=plain)
    raw = ops.edge_bce_loss_raw(t.Ud, t.Pd, g.ei_d, sk, g.E, t.wd.mean(), neg_order="user",
                                presorted=pre)
    close(raw[0], _ref(g, t, k, "mean")[0])
    close(raw[2] * UP, _ref(g, t, k, "mean")[2])
