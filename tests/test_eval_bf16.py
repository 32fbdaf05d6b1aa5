"""bf16 rows in ``evaluate`` / ``recommend``: the fused scoring on bf16 MFMA (hgnn_score_topk_bf16,
csrc/eval.hip) and the Python surface around it.  The mode's contract: every result is what the
fp32 path returns on R(U), R(P), R(T) = T.to(bfloat16).float().  Integers of magnitude <= 60 are
exact in bf16 and their dot products stay far below 2^24, so on such data the bf16 path must give
the exact CPU ranking."""
import inspect
import pathlib
import re

import numpy as np
import pytest
import torch

from oracle import eval_ref
from truth_recommendation_gnn_amd import _native as N
from truth_recommendation_gnn_amd import evaluate, recommend

ROOT = pathlib.Path(__file__).resolve().parents[1]
DEV = torch.device("cuda")
NEW = ("hgnn_score_topk_bf16", "hgnn_score_topk_bf16_lds_bytes")


def R(t):
    return t.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------- CPU
def test_header_declares_and_ctypes_binds_the_bf16_entries():
    text = (ROOT / "include" / "hgnn.h").read_text()
    lib = N.lib()
    for name in NEW:
        m = re.search(r"^\w[\w\s\*]*?\b%s\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, f"{name} not declared in include/hgnn.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in N._SIGS
        assert len(N._SIGS[name][1]) == n_args
        assert hasattr(lib, name)
    # the bf16 entry takes hgnn_score_topk's arguments, position by position
    assert N._SIGS["hgnn_score_topk_bf16"] == N._SIGS["hgnn_score_topk"]
    assert N._SIGS["hgnn_score_topk_bf16_lds_bytes"] == N._SIGS["hgnn_score_topk_lds_bytes"]


def test_row_dtype_on_cpu_tensors_is_a_value_error():
    U, P = torch.ones(3, 64), torch.ones(5, 64)
    te = torch.tensor([[0, 1], [3, 4]])
    with pytest.raises(ValueError, match="ROCm GPU"):
        recommend(U, P, row_dtype="bf16")
    with pytest.raises(ValueError, match="ROCm GPU"):
        evaluate(te, U, P, row_dtype="bf16")
    with pytest.raises(ValueError, match="ROCm GPU"):
        recommend(U.bfloat16(), P.bfloat16())


def test_unknown_row_dtype_is_a_value_error():
    U, P = torch.ones(3, 64), torch.ones(5, 64)
    with pytest.raises(ValueError, match="fp8"):
        recommend(U, P, row_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        evaluate(torch.tensor([[0], [3]]), U, P, row_dtype="fp8")


def test_row_dtype_default_is_fp32_not_the_environment():
    for fn in (evaluate, recommend):
        assert inspect.signature(fn).parameters["row_dtype"].default == "fp32"


def test_dtype_combinations_that_are_type_errors():
    U, P = torch.ones(3, 64), torch.ones(5, 64)
    for a, b, kw in ((U.bfloat16(), P, {}), (U, P.bfloat16(), {"row_dtype": "bf16"}),
                     (U.bfloat16(), P.bfloat16(), {"row_dtype": "fp32"}),
                     (U.half(), P.half(), {}), (U.double(), P.double(), {"row_dtype": "bf16"})):
        with pytest.raises(TypeError):
            recommend(a, b, **kw)
        with pytest.raises(TypeError):
            evaluate(torch.tensor([[0], [3]]), a, b, **kw)


def _chunk_rows(d, L):
    """Candidates per chunk of the (d, L) launch, from its LDS bytes: the lists of a workgroup's
    128 users, and two bf16 chunk buffers of rows padded by 16 halfwords."""
    b = N.lib().hgnn_score_topk_bf16_lds_bytes(d, L)
    rows, rest = divmod(b - 128 * L * 8, 2 * (d + 16) * 2)
    assert rest == 0, (d, L, b)
    return rows


def test_lds_bytes_fit_one_cu_for_every_legal_list_length():
    lib = N.lib()
    for d in (64, 128):
        for L in range(1, 65):
            assert lib.hgnn_score_topk_bf16_lds_bytes(d, L) <= 160 * 1024, (d, L)
            assert _chunk_rows(d, L) in (32, 64), (d, L)


# ----------------------------------------------------------------------------- GPU
def _ints(seed, n, C, d, lo=-3, hi=4):
    rng = np.random.default_rng(seed)
    U = torch.from_numpy(rng.integers(lo, hi, size=(n, d)).astype(np.float32))
    P = torch.from_numpy(rng.integers(lo, hi, size=(C, d)).astype(np.float32))
    return U, P


def _exact_lists(S, k):
    C = S.shape[1]
    return [sorted(range(C), key=lambda j, row=row: (-row[j], j))[:k] for row in S.tolist()]


def _assert_exact(s, i, S, k):
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    assert s.shape == (S.shape[0], k) and i.shape == (S.shape[0], k)
    for r, order in enumerate(_exact_lists(S, k)):
        assert i[r].tolist() == order, r
        assert torch.equal(s[r].cpu(), S[r, order]), r


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("n,C,K", [(50, 1000, 10), (3, 7, 10), (300, 4097, 25), (129, 65, 63),
                                   (257, 64, 1), (40, 64, 64), (520, 300, 40)])
def test_recommend_bf16_exact(n, C, K, d):
    """n not a multiple of the block's 128 users (below it, several blocks), C = a chunk +- 1
    and less than one, L = 1 and L = 64."""
    U, P = _ints(C + d, n, C, d, lo=-60, hi=61)
    S = U @ P.T
    k = min(K, C)
    Ud, Pd = U.to(DEV), P.to(DEV)
    s, i = recommend(Ud, Pd, K, row_dtype="bf16")
    _assert_exact(s, i, S, k)
    s32, i32 = recommend(Ud, Pd, K, row_dtype="fp32")
    assert torch.equal(s, s32) and torch.equal(i, i32)
    sb, ib = recommend(Ud.bfloat16(), Pd.bfloat16(), K)
    assert torch.equal(s, sb) and torch.equal(i, ib)
    sb, ib = recommend(Ud.bfloat16(), Pd.bfloat16(), K, row_dtype="bf16")
    assert torch.equal(s, sb) and torch.equal(i, ib)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("n,C", [(3, 7), (129, 65), (3, 65), (129, 7)])
def test_recommend_bf16_never_returns_padding(n, C, d):
    """Every score is negative, so a zero row past the candidates (chunk padding) would win."""
    rng = np.random.default_rng(n * C)
    U = torch.from_numpy(rng.integers(1, 8, size=(n, d)).astype(np.float32))
    P = torch.from_numpy(-rng.integers(1, 8, size=(C, d)).astype(np.float32))
    S = U @ P.T
    assert float(S.max()) < 0
    for K in (5, 64):
        k = min(K, C)
        s, i = recommend(U.to(DEV), P.to(DEV), K, row_dtype="bf16")
        assert int(i.max()) < C and int(i.min()) >= 0
        _assert_exact(s, i, S, k)


def _raw(entry, U, rows, n_rows, P, C, d, L):
    topv = torch.full((n_rows, L), float("nan"), device=DEV)
    topi = torch.full((n_rows, L), -1, dtype=torch.int32, device=DEV)
    N.check(getattr(N.lib(), entry)(N.ptr(U), N.ptr(rows), n_rows, N.ptr(P), C, d, L,
                                    N.ptr(topv), N.ptr(topi), N.stream_ptr(DEV)), entry)
    return topv.cpu(), topi.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_raw_entry_follows_the_rows_indirection(d):
    U, P = _ints(d, 40, 333, d, lo=-60, hi=61)
    rng = np.random.default_rng(5)
    n_rows, L = 130, 11
    rows = torch.from_numpy(np.concatenate([rng.permutation(40), rng.integers(0, 40, 90)])
                            .astype(np.int32))
    Ud, Pd, rd = U.to(DEV), P.to(DEV), rows.to(DEV)
    v32, i32 = _raw("hgnn_score_topk", Ud, rd, n_rows, Pd, 333, d, L)
    vb, ib = _raw("hgnn_score_topk_bf16", Ud.bfloat16(), rd, n_rows, Pd.bfloat16(), 333, d, L)
    assert torch.equal(vb, v32) and torch.equal(ib, i32)
    S = U[rows.long()] @ P.T
    for r, order in enumerate(_exact_lists(S, L)):
        assert ib[r].tolist() == order


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_raw_entry_at_every_change_of_chunk(d):
    """The candidates per chunk follow (d, L): list lengths on both sides of each L at which the
    launch changes, the shortest and the longest list, over several ragged blocks."""
    Ls = sorted({1, 2, 64} | {L + o for L in range(1, 64) for o in (0, 1)
                              if _chunk_rows(d, L) != _chunk_rows(d, L + 1)})
    assert len(Ls) > 3 and {_chunk_rows(d, L) for L in Ls} == {32, 64}
    U, P = _ints(d + 1, 64, 200, d, lo=-60, hi=61)
    rng = np.random.default_rng(6)
    n_rows = 300
    rows = torch.from_numpy(rng.integers(0, 64, n_rows).astype(np.int32))
    Ud, Pd, rd = U.to(DEV), P.to(DEV), rows.to(DEV)
    Ub, Pb = Ud.bfloat16(), Pd.bfloat16()
    for L in Ls:
        v32, i32 = _raw("hgnn_score_topk", Ud, rd, n_rows, Pd, 200, d, L)
        vb, ib = _raw("hgnn_score_topk_bf16", Ub, rd, n_rows, Pb, 200, d, L)
        assert torch.equal(ib, i32), L
        assert torch.equal(vb, v32), L


@pytest.mark.gpu
def test_raw_entry_argument_checks_match_the_fp32_entry():
    U = torch.zeros(4, 64, device=DEV)
    Ub = U.bfloat16()
    lib = N.lib()
    out_v = torch.empty(4, 64, device=DEV)
    out_i = torch.empty(4, 64, dtype=torch.int32, device=DEV)

    def rc(entry, T, n_cand, d, L, off=0):
        p = N._p(T.data_ptr() + off)
        return getattr(lib, entry)(p, None, 4, p, n_cand, d, L, N.ptr(out_v), N.ptr(out_i),
                                   N.stream_ptr(DEV))
    for n_cand, d, L, off in ((4, 64, 5, 0), (4, 64, 0, 0), (4, 64, 65, 0), (0, 64, 1, 0),
                              (4, 32, 2, 0), (4, 96, 2, 0), (4, 64, 2, 8)):
        want = rc("hgnn_score_topk", U, n_cand, d, L, off)
        assert want != 0
        assert rc("hgnn_score_topk_bf16", Ub, n_cand, d, L, off) == want


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("n_users,n_posts,E,K", [(300, 257, 3000, 10), (64, 7, 200, 10),
                                                 (500, 1000, 2500, 1), (200, 90, 800, 33),
                                                 (150, 700, 1500, 63)])
def test_evaluate_bf16_matches_reference_loop_exact_scores(n_users, n_posts, E, K, d):
    """Small integers: full of ties, so most rows are redone on the materialised path from the
    widened bf16 rows; the rest finish from the fused bf16 lists."""
    from test_eval import _int_case
    U, P, te = _int_case(n_users + K, n_users, n_posts, E, d, extra_users=5)
    users, rec, nd = eval_ref.evaluate(te, U, P, n_users, K=K, tie_break="index", per_user=True)
    for Ux, Px, kw in ((U, P, {"row_dtype": "bf16"}), (U.bfloat16(), P.bfloat16(), {})):
        r, n = evaluate(te.to(DEV), Ux.to(DEV), Px.to(DEV), K=K, fused=True, **kw)
        assert abs(r - float(np.mean(rec))) < 1e-12
        assert abs(n - float(np.mean(nd))) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_evaluate_bf16_without_ties_matches_reference(d):
    from test_eval import _int_case
    U, P, te = _int_case(d, 400, 3000, 6000, d, lo=-60, hi=61)
    users, rec, nd = eval_ref.evaluate(te, U, P, 400, K=10, tie_break="index", per_user=True)
    r, n = evaluate(te.to(DEV), U.to(DEV), P.to(DEV), K=10, fused=True, row_dtype="bf16")
    assert abs(r - float(np.mean(rec))) < 1e-12
    assert abs(n - float(np.mean(nd))) < 1e-12


@pytest.mark.gpu
def test_recommend_bf16_continuous_data():
    """randn tables: against float64 scores of the rounded rows, at the project's fp32 bar."""
    g = torch.Generator().manual_seed(11)
    n, C, K, d = 200, 1500, 10, 128
    U, P = torch.randn(n, d, generator=g), torch.randn(C, d, generator=g)
    ref = R(U).double() @ R(P).double().T
    s, i = recommend(U.to(DEV), P.to(DEV), K, row_dtype="bf16")
    s, i = s.cpu().double(), i.cpu()
    atol = 1e-5 * float(ref.abs().max())
    got_ref = ref.gather(1, i)
    tol = atol + 1e-4 * got_ref.abs()
    err = (s - got_ref).abs()
    print(f"max |score - ref| = {float(err.max()):.3e} (tolerance >= {atol:.3e})")
    assert bool((err <= tol).all())
    assert bool((s[:, :-1] >= s[:, 1:]).all())                      # sorted
    assert all(len(set(row.tolist())) == K for row in i)            # K distinct candidates
    kth = ref.topk(K, dim=1).values[:, -1:]
    assert bool((got_ref >= kth - (atol + 1e-4 * kth.abs())).all())   # no row excused


def _rounding_case(d):
    """Scores that are single table entries or sums of two, on a 2^-10 grid in [1, 2): exact in
    fp32 in any summation order, and collapsing onto bf16's 2^-7 grid changes the ranking."""
    rng = np.random.default_rng(d)
    n, C = 70, 400
    U = torch.zeros(n, d)
    for r in range(n):
        U[r, r % d] = 1.0
        if r % 3 == 0:
            U[r, (r * 7 + 1) % d] = 2.0
    P = torch.from_numpy(1.0 + rng.integers(0, 1024, size=(C, d)).astype(np.float32) / 1024.0)
    return U, P


def _edges_to_fp32_winners(full, n_users):
    """Test edges user -> each of its top-K posts in the fp32 ranking: Recall@K is exactly 1 on
    the tables as given and lower wherever the rounded rows rank another set."""
    u = np.repeat(np.arange(len(full)), len(full[0]))
    p = n_users + np.asarray(full).reshape(-1)
    return torch.from_numpy(np.stack([u, p]).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_bf16_rounding_is_applied(d):
    U, P = _rounding_case(d)
    K = 10
    full = _exact_lists(U @ P.T, K)
    rounded = _exact_lists(R(U) @ R(P).T, K)
    # R changes the order of most rows' lists and the membership of many
    assert sum(a != b for a, b in zip(full, rounded)) > len(full) // 2
    assert sum(set(a) != set(b) for a, b in zip(full, rounded)) >= 10
    Ud, Pd = U.to(DEV), P.to(DEV)
    s, i = recommend(Ud, Pd, K, row_dtype="bf16")
    sr, ir = recommend(R(Ud), R(Pd), K)
    s32, i32 = recommend(Ud, Pd, K)
    assert torch.equal(i, ir) and torch.equal(s, sr)
    assert i.cpu().tolist() == rounded
    assert not torch.equal(i, i32)
    assert i32.cpu().tolist() == full
    # evaluate: the metrics are those of the rounded rows, not of the tables as given
    te = _edges_to_fp32_winners(full, U.shape[0]).to(DEV)
    got = evaluate(te, Ud, Pd, K=K, row_dtype="bf16")
    assert got == evaluate(te, R(Ud), R(Pd), K=K)
    assert got[0] < 1.0 == evaluate(te, Ud, Pd, K=K)[0]


@pytest.mark.gpu
def test_other_widths_score_the_rounded_rows():
    """d = 16 takes the materialised path: on R(U), R(P), not on U, P."""
    U, P = _rounding_case(16)
    K = 10
    full = _exact_lists(U @ P.T, K)
    rounded = _exact_lists(R(U) @ R(P).T, K)
    # R changes the order of most rows' lists and the membership of many
    assert sum(a != b for a, b in zip(full, rounded)) > len(full) // 2
    assert sum(set(a) != set(b) for a, b in zip(full, rounded)) >= 10
    Ud, Pd = U.to(DEV), P.to(DEV)
    sr, ir = recommend(R(Ud), R(Pd), K)
    assert ir.cpu().tolist() == rounded
    for Ux, Px, kw in ((Ud, Pd, {"row_dtype": "bf16"}), (Ud.bfloat16(), Pd.bfloat16(), {})):
        s, i = recommend(Ux, Px, K, **kw)
        assert s.dtype == torch.float32
        assert torch.equal(i, ir) and torch.equal(s, sr)
    te = _edges_to_fp32_winners(full, U.shape[0]).to(DEV)
    got = evaluate(te, Ud, Pd, K=K, row_dtype="bf16")
    assert got == evaluate(te, R(Ud), R(Pd), K=K)
    assert got == evaluate(te, Ud.bfloat16(), Pd.bfloat16(), K=K)
    assert got[0] < 1.0 == evaluate(te, Ud, Pd, K=K)[0]
