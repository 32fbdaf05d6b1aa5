"""``recommend(..., users=, exclude=)``: seen-post exclusion and user subsets inside the fused top-K
(hgnn_score_topk_excl, hgnn_score_topk_excl_bf16, csrc/eval.hip), ``metrics.SeenIndex``, and the
materialised path beside them.  Integer tables with entries in [-60, 60] make every score exact in
fp32 and in bf16, so the reference is an exact CPU one: S = U[users] @ P.T, -inf at the excluded
posts, order by (-score, index), and -inf entries leave as (-inf, -1)."""
import ctypes
import math
import pathlib
import re

import numpy as np
import pytest
import torch

import truth_recommendation_gnn_amd as pkg
from truth_recommendation_gnn_amd import _native as N
from truth_recommendation_gnn_amd import metrics, recommend

ROOT = pathlib.Path(__file__).resolve().parents[1]
DEV = torch.device("cuda")
NEW = ("hgnn_score_topk_excl", "hgnn_score_topk_excl_bf16")
HGNN_E_ARG = 1001


# ----------------------------------------------------------------------------- CPU
def test_header_declares_and_ctypes_binds_the_excluding_entries():
    text = (ROOT / "include" / "hgnn.h").read_text()
    lib = N.lib()
    for name in NEW:
        m = re.search(r"^\w[\w\s\*]*?\b%s\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, f"{name} not declared in include/hgnn.h"
        args = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert name in N._SIGS
        assert len(N._SIGS[name][1]) == len(args) == 13
        assert [a.split()[-1].lstrip("*") for a in args[7:10]] == ["excl_rowptr", "excl_col",
                                                                   "excl_rows"]
        assert hasattr(lib, name)
    assert N._SIGS["hgnn_score_topk_excl_bf16"] == N._SIGS["hgnn_score_topk_excl"]
    # the plain entry's arguments with the three exclusion pointers in front of the outputs
    plain = N._SIGS["hgnn_score_topk"][1]
    assert N._SIGS["hgnn_score_topk_excl"][1] == plain[:7] + [ctypes.c_void_p] * 3 + plain[7:]
    assert "hgnn_topk_finish" in text.split("hgnn_score_topk_excl(")[0].rsplit("/*", 1)[1]


def test_lds_bytes_entries_are_pinned():
    """The dynamic LDS of a launch, as the two queries report it: two chunk buffers of padded rows
    and 128 lists.  fp32: chunks of 64 rows of d + 8 dwords.  bf16: rows of d + 16 halfwords in
    chunks of 64, or of 32 where that lets one more workgroup live on the CU (at most 4, or 3 for
    the d = 128, 64-row kernel, and what 160 KiB hold); never more than 100 KiB."""
    lib = N.lib()
    # 2 * chunk * (d + 16) * 2 + 128 * L * 8 with the chunks 64, 64, 32 (d = 64), 32, 32, 64 (128)
    bf16 = {(64, 1): 21504, (64, 11): 31744, (64, 64): 75776,
            (128, 1): 19456, (128, 11): 29696, (128, 64): 102400}
    for (d, L), want in bf16.items():
        assert lib.hgnn_score_topk_lds_bytes(d, L) == 2 * 64 * (d + 8) * 4 + 128 * L * 8
        assert lib.hgnn_score_topk_bf16_lds_bytes(d, L) == want, (d, L)
        assert want <= 100 * 1024


def test_cpu_tensors_are_a_value_error():
    U, P = torch.ones(3, 64), torch.ones(5, 64)
    edges = torch.tensor([[0, 1], [3, 4]])
    with pytest.raises(ValueError, match="ROCm GPU"):
        metrics.SeenIndex(edges, 3, 5)
    with pytest.raises(ValueError, match="ROCm GPU"):
        recommend(U, P, exclude=edges)
    with pytest.raises(ValueError, match="ROCm GPU"):
        recommend(U, P, users=torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="ROCm GPU"):
        recommend(U, P, users=torch.tensor([0, 2]), exclude=edges, row_dtype="bf16")


def test_seen_index_is_exported():
    assert pkg.SeenIndex is metrics.SeenIndex


# ----------------------------------------------------------------------------- GPU
def _ints(seed, n, C, d, dup=True):
    """Integer tables in [-60, 60].  With ``dup`` post C // 2 + j repeats post j, so every score
    of the lower half ties one of the upper half and the lower-index rule shows in every list."""
    rng = np.random.default_rng(seed)
    U = torch.from_numpy(rng.integers(-60, 61, size=(n, d)).astype(np.float32))
    P = torch.from_numpy(rng.integers(-60, 61, size=(C, d)).astype(np.float32))
    if dup:
        h = C // 2
        P[h:2 * h] = P[:h]
    return U, P


def _lists(S, K, seed):
    """One exclusion list per user (row of S = U @ P.T), the kinds by user id modulo 7."""
    rng = np.random.default_rng(seed)
    n_u, C = S.shape
    out = []
    for u in range(n_u):
        kind = u % 7
        order = torch.sort(S[u], descending=True, stable=True).indices.tolist()
        if kind == 0:      # the row's global best, and a few others
            x = {order[0]} | set(rng.integers(0, C, 3).tolist())
        elif kind == 1:    # the lower index of the best tied pair: its twin takes the place
            tied = [r for r in range(C - 1) if S[u, order[r]] == S[u, order[r + 1]]]
            x = {order[tied[0]]} if tied else {order[0]}
        elif kind == 2:    # nothing
            x = set()
        elif kind == 3:    # the chunk edges of both chunk sizes
            x = {c for c in (0, 31, 32, 63, 64, C - 1) if c < C}
        elif kind == 4:    # fewer than K candidates left
            x = set(range(C)) - set(rng.permutation(C)[:min(K - 1, 3)].tolist())
        elif kind == 5:    # every candidate
            x = set(range(C))
        else:              # about a third of the posts
            x = set(np.nonzero(rng.random(C) < 0.3)[0].tolist())
        out.append(sorted(x))
    return out


def _edges(lists, seed, dev=DEV):
    """[2, M] (user, post) pairs of the lists, shuffled, with some pairs repeated."""
    rng = np.random.default_rng(seed)
    pairs = [(u, c) for u, l in enumerate(lists) for c in l]
    pairs += [pairs[j] for j in rng.integers(0, max(len(pairs), 1), len(pairs) // 3)] if pairs \
        else []
    e = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[rng.permutation(len(pairs))]
    return torch.from_numpy(np.ascontiguousarray(e.T)).to(dev)


def _reference(U, P, users, lists, K):
    """Exact CPU lists: (scores [n, k] fp32, indices [n, k] int64)."""
    users = list(range(U.shape[0])) if users is None else [int(u) for u in users]
    S = U[users] @ P.T
    for r, u in enumerate(users):
        S[r, lists[u]] = -math.inf
    k = min(K, P.shape[0])
    v, i = torch.sort(S, dim=1, descending=True, stable=True)   # equal scores: lower index first
    v, i = v[:, :k].contiguous(), i[:, :k].contiguous()
    i[v == -math.inf] = -1
    return v, i


def _same(got, want):
    s, i = got
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(i.cpu(), want[1])
    assert torch.equal(s.cpu(), want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("K", [1, 10, 64])
@pytest.mark.parametrize("C", [7, 64, 65, 200])
@pytest.mark.parametrize("n", [3, 129, 300])
def test_recommend_exclude_exact(n, C, K, d):
    """n below, just over and several times the 128-user workgroup (ragged waves at 32 and at 16
    users per wave); C less than a chunk, one 64-chunk, one more, several ragged ones."""
    n_u = n + 4
    U, P = _ints(1000 * n + 10 * C + d + K, n_u, C, d)
    lists = _lists(U @ P.T, K, n + C)
    rng = np.random.default_rng(n * C + K)
    users = rng.permutation(n_u)[:n]
    users[0], users[1] = 5, 0                              # everything excluded; the best excluded
    users[-1] = users[0]                                   # one user twice
    Ud, Pd, ud = U.to(DEV), P.to(DEV), torch.from_numpy(users).to(DEV)
    seen = metrics.SeenIndex(_edges(lists, d + K), n_u, C)
    want = _reference(U, P, users, lists, K)
    assert bool((want[1] == -1).any()) and bool((want[1][:, 0] >= 0).any())
    got = recommend(Ud, Pd, K, users=ud, exclude=seen)
    _same(got, want)
    for Ux, Px, kw in ((Ud, Pd, {"row_dtype": "bf16"}), (Ud.bfloat16(), Pd.bfloat16(), {})):
        gb = recommend(Ux, Px, K, users=ud, exclude=seen, **kw)
        assert torch.equal(gb[0], got[0]) and torch.equal(gb[1], got[1])   # bitwise, both formats
    # every row of the table (users=None), the index built for the call from the edges
    want_all = _reference(U, P, None, lists, K)
    _same(recommend(Ud, Pd, K, exclude=_edges(lists, 3)), want_all)
    _same(recommend(Ud, Pd, K, exclude=seen, row_dtype="bf16"), want_all)


def _raw(entry, U, rows, n_rows, P, C, d, L, excl=None):
    topv = torch.full((n_rows, L), float("nan"), device=DEV)
    topi = torch.full((n_rows, L), -7, dtype=torch.int32, device=DEV)
    mid = () if excl is None else tuple(N.ptr(t) for t in excl)
    N.check(getattr(N.lib(), entry)(N.ptr(U), N.ptr(rows), n_rows, N.ptr(P), C, d, L, *mid,
                                    N.ptr(topv), N.ptr(topi), N.stream_ptr(DEV)), entry)
    return topv.cpu(), topi.cpu()


def _chunk_rows(d, L):
    """Candidates per chunk of the plain bf16 (d, L) launch, from its LDS bytes."""
    b = N.lib().hgnn_score_topk_bf16_lds_bytes(d, L)
    rows, rest = divmod(b - 128 * L * 8, 2 * (d + 16) * 2)
    assert rest == 0, (d, L, b)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_raw_entries_at_every_list_length(d):
    """The bf16 launch changes its chunk (32 or 64 candidates) with (d, L), and the excluding
    kernels, which hold more registers, at other L than the plain ones: every L from 1 to 64, the
    plain launch's switches among them, with exclusions on, over several ragged blocks."""
    switches = {L + o for L in range(1, 64) for o in (0, 1)
                if _chunk_rows(d, L) != _chunk_rows(d, L + 1)}
    assert switches and switches <= set(range(1, 65))
    n_u, n_rows, C = 64, 300, 200
    U, P = _ints(d + 2, n_u, C, d)
    lists = _lists(U @ P.T, 10, d)
    seen = metrics.SeenIndex(_edges(lists, d), n_u, C)
    rng = np.random.default_rng(7)
    rows = rng.integers(0, n_u, n_rows).astype(np.int32)
    Ud, Pd, rd = U.to(DEV), P.to(DEV), torch.from_numpy(rows).to(DEV)
    Ub, Pb = Ud.bfloat16(), Pd.bfloat16()
    excl = (seen.rowptr, seen.col, rd)
    full = _reference(U, P, rows, lists, 64)
    for L in range(1, 65):
        v32, i32 = _raw("hgnn_score_topk_excl", Ud, rd, n_rows, Pd, C, d, L, excl)
        vb, ib = _raw("hgnn_score_topk_excl_bf16", Ub, rd, n_rows, Pb, C, d, L, excl)
        assert torch.equal(i32.long(), full[1][:, :L]), L
        assert torch.equal(v32, full[0][:, :L]), L
        assert torch.equal(ib, i32) and torch.equal(vb, v32), L


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_raw_entries_follow_rows_and_excl_rows_independently(d):
    n_u, n_rows, C, L = 40, 130, 333, 11
    U, P = _ints(d, n_u, C, d)
    lists = _lists(U @ P.T, L, 1)
    seen = metrics.SeenIndex(_edges(lists, 2), n_u, C)
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.permutation(n_u), rng.integers(0, n_u, n_rows - n_u)])
    erows = rng.integers(0, n_u, n_rows)
    rd = torch.from_numpy(rows.astype(np.int32)).to(DEV)
    ed = torch.from_numpy(erows.astype(np.int32)).to(DEV)
    Ud, Pd = U.to(DEV), P.to(DEV)
    Ur = Ud.index_select(0, rd).contiguous()               # rows = NULL: U holds the output rows
    # excl_rows = NULL: one list per output row, here those of users erows[r]
    direct = metrics.SeenIndex(_edges([lists[e] for e in erows], 3), n_rows, C)
    S = U[rows] @ P.T
    for r, e in enumerate(erows):
        S[r, lists[e]] = -math.inf
    v, i = torch.sort(S, dim=1, descending=True, stable=True)
    v, i = v[:, :L].contiguous(), i[:, :L].contiguous()
    i[v == -math.inf] = -1
    for entry, cast in (("hgnn_score_topk_excl", lambda t: t),
                        ("hgnn_score_topk_excl_bf16", lambda t: t.bfloat16())):
        for Ux, rx, ex in ((Ud, rd, (seen.rowptr, seen.col, ed)),
                           (Ur, None, (seen.rowptr, seen.col, ed)),
                           (Ud, rd, (direct.rowptr, direct.col, None)),
                           (Ur, None, (direct.rowptr, direct.col, None))):
            gv, gi = _raw(entry, cast(Ux), rx, n_rows, cast(Pd), C, d, L, ex)
            assert torch.equal(gi.long(), i), (entry, rx is None, ex[2] is None)
            assert torch.equal(gv, v)


@pytest.mark.gpu
def test_raw_entries_argument_checks():
    U = torch.zeros(4, 64, device=DEV)
    Ub = U.bfloat16()
    lib = N.lib()
    out_v = torch.empty(4, 64, device=DEV)
    out_i = torch.empty(4, 64, dtype=torch.int32, device=DEV)
    rowptr = torch.zeros(5, dtype=torch.int32, device=DEV)
    col = torch.zeros(1, dtype=torch.int32, device=DEV)

    def rc(entry, T, n_cand, d, L, off=0, excl=None, n_rows=4):
        p = N._p(T.data_ptr() + off)
        mid = () if excl is None else tuple(N.ptr(t) for t in excl)
        return getattr(lib, entry)(p, None, n_rows, p, n_cand, d, L, *mid, N.ptr(out_v),
                                   N.ptr(out_i), N.stream_ptr(DEV))
    ok = (rowptr, col, None)
    for n_cand, d, L, off in ((4, 64, 5, 0), (4, 64, 0, 0), (4, 64, 65, 0), (0, 64, 1, 0),
                              (4, 32, 2, 0), (4, 96, 2, 0), (4, 64, 2, 8)):
        want = rc("hgnn_score_topk", U, n_cand, d, L, off)
        assert want != 0
        assert rc("hgnn_score_topk_excl", U, n_cand, d, L, off, ok) == want
        assert rc("hgnn_score_topk_excl_bf16", Ub, n_cand, d, L, off, ok) == want
    for entry, T in (("hgnn_score_topk_excl", U), ("hgnn_score_topk_excl_bf16", Ub)):
        assert rc(entry, T, 4, 64, 2, 0, ok) == 0
        assert rc(entry, T, 4, 64, 2, 0, (None, col, None)) == HGNN_E_ARG
        assert rc(entry, T, 4, 64, 2, 0, (rowptr, None, None)) == HGNN_E_ARG
        assert rc(entry, T, 4, 64, 2, 0, (None, None, None)) == HGNN_E_ARG
        assert rc(entry, T, 4, 64, 2, 0, (None, col, None), n_rows=0) == HGNN_E_ARG
        assert rc(entry, T, 4, 64, 2, 0, ok, n_rows=0) == 0
        assert rc(entry, T, 4, 64, 2, 0, ok, n_rows=-1) == HGNN_E_ARG


@pytest.mark.gpu
def test_users_are_keys_of_the_exclusion_lists():
    """Repeats and a permutation in ``users``; the lists follow the user id, not the position; a
    user with exclusions that is not asked for changes nothing."""
    n_u, C, K, d = 150, 200, 10, 64
    U, P = _ints(9, n_u, C, d)
    lists = _lists(U @ P.T, K, 4)
    Ud, Pd = U.to(DEV), P.to(DEV)
    rng = np.random.default_rng(12)
    asked = rng.permutation(n_u)[:100]
    users = np.concatenate([asked, asked[:40][::-1], asked[5:6].repeat(3)])
    ud = torch.from_numpy(users).to(DEV)
    seen = metrics.SeenIndex(_edges(lists, 5), n_u, C)
    got = recommend(Ud, Pd, K, users=ud, exclude=seen)
    _same(got, _reference(U, P, users, lists, K))
    pos = {int(u): r for r, u in enumerate(users[:100])}
    for r in range(100, len(users)):                       # a repeated user: the same list again
        assert torch.equal(got[1][r], got[1][pos[int(users[r])]])
        assert torch.equal(got[0][r], got[0][pos[int(users[r])]])
    others = [l if u in pos else [] for u, l in enumerate(lists)]
    assert others != lists
    again = recommend(Ud, Pd, K, users=ud, exclude=metrics.SeenIndex(_edges(others, 6), n_u, C))
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    # int32 users, users alone (no exclusion), an empty subset
    _same(recommend(Ud, Pd, K, users=ud.int(), exclude=seen), _reference(U, P, users, lists, K))
    none = [[] for _ in lists]
    for kw in ({}, {"row_dtype": "bf16"}):
        _same(recommend(Ud, Pd, K, users=ud, **kw), _reference(U, P, users, none, K))
    s, i = recommend(Ud, Pd, K, users=ud[:0], exclude=seen)
    assert s.shape == (0, K) and i.shape == (0, K) and i.dtype == torch.int64


@pytest.mark.gpu
def test_bad_arguments_are_value_errors():
    U, P = torch.ones(6, 64, device=DEV), torch.ones(9, 64, device=DEV)
    edges = torch.tensor([[0, 5], [8, 0]], device=DEV)
    for bad in ([[0, 6], [8, 0]], [[0, -1], [8, 0]], [[0, 5], [9, 0]], [[0, 5], [-1, 0]]):
        with pytest.raises(ValueError):
            metrics.SeenIndex(torch.tensor(bad, device=DEV), 6, 9)
        with pytest.raises(ValueError):
            recommend(U, P, exclude=torch.tensor(bad, device=DEV))
    with pytest.raises(ValueError):
        metrics.SeenIndex(torch.ones(2, 3, device=DEV), 6, 9)          # not integers
    with pytest.raises(ValueError):
        metrics.SeenIndex(torch.ones(3, 2, dtype=torch.int64, device=DEV), 6, 9)
    for nu, npst in ((7, 9), (6, 10)):                                 # built for other tables
        with pytest.raises(ValueError):
            recommend(U, P, exclude=metrics.SeenIndex(edges, nu, npst))
    for bad in ([0, 6], [-1, 2]):
        with pytest.raises(ValueError):
            recommend(U, P, users=torch.tensor(bad, device=DEV))
    with pytest.raises(ValueError):
        recommend(U, P, users=torch.tensor([0.0, 1.0], device=DEV))
    with pytest.raises(ValueError):
        recommend(U, P, users=torch.tensor([0, 1]))                    # a CPU tensor
    recommend(U, P, users=torch.tensor([0, 5], device=DEV), exclude=edges)


@pytest.mark.gpu
def test_seen_index_equals_the_numpy_grouping():
    rng = np.random.default_rng(21)
    n_u, n_p, M = 70, 50, 900
    e = np.stack([rng.integers(0, n_u, M), rng.integers(0, n_p, M)])
    e[:, 600:] = e[:, :300]                                            # duplicates
    e[0, e[0] == 13] = 14                                              # a user without edges
    e = e[:, rng.permutation(M)]
    seen = metrics.SeenIndex(torch.from_numpy(e).to(DEV), n_u, n_p)
    pairs = np.unique(e.T, axis=0)                                     # sorted by (user, post)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n_u))])
    assert seen.rowptr.dtype == torch.int32 and seen.col.dtype == torch.int32
    assert seen.rowptr.device.type == "cuda" and seen.col.is_contiguous()
    assert seen.rowptr.cpu().tolist() == rowptr.tolist()
    assert seen.col.cpu().tolist() == pairs[:, 1].tolist()
    assert rowptr[14] == rowptr[13]
    for dt in (torch.int32, torch.int64):                              # and no edges at all
        empty = metrics.SeenIndex(torch.empty(2, 0, dtype=dt, device=DEV), n_u, n_p)
        assert empty.rowptr.cpu().tolist() == [0] * (n_u + 1) and empty.col.numel() == 0
    U, P = _ints(3, n_u, n_p, 64)
    _same(recommend(U.to(DEV), P.to(DEV), 5, exclude=empty),
          _reference(U, P, None, [[] for _ in range(n_u)], 5))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_excluding_list_is_the_plain_list_with_the_entries_removed(d):
    """Continuous data, library against library: for rows with |excluded| + L <= 64 the excluding
    list is the plain list of length L + |excluded| without the excluded entries, cut to L;
    bitwise, values too, because the same MFMA sums feed both."""
    g = torch.Generator().manual_seed(d)
    n, C, L = 300, 1000, 10
    U, P = torch.randn(n, d, generator=g), torch.randn(C, d, generator=g)
    rng = np.random.default_rng(d)
    top = (U @ P.T).topk(40, dim=1).indices.numpy()
    lists = []
    for r in range(n):                                     # mostly posts that would be listed
        m = int(rng.integers(0, 55)) if r % 9 else 0
        x = set(rng.choice(top[r], size=min(m, 30), replace=False).tolist())
        x |= set(rng.integers(0, C, max(0, m - len(x))).tolist())
        lists.append(sorted(x))
    seen = metrics.SeenIndex(_edges(lists, 8), n, C)
    Ud, Pd = U.to(DEV), P.to(DEV)
    for entry, cast in (("hgnn_score_topk", lambda t: t),
                        ("hgnn_score_topk_bf16", lambda t: t.bfloat16())):
        Ux, Px = cast(Ud).contiguous(), cast(Pd).contiguous()
        ev, ei = _raw(entry.replace("topk", "topk_excl"), Ux, None, n, Px, C, d, L,
                      (seen.rowptr, seen.col, None))
        plain = {}
        checked = 0
        for r in range(n):
            m = len(lists[r])
            assert m + L <= 64
            if m not in plain:
                plain[m] = _raw(entry, Ux, None, n, Px, C, d, L + m)
            pv, pi = plain[m]
            keep = [j for j in range(L + m) if int(pi[r, j]) not in set(lists[r])][:L]
            assert ei[r].tolist() == pi[r, keep].tolist(), (entry, r)
            assert torch.equal(ev[r], pv[r, keep]), (entry, r)
            checked += m > 0 and len(keep) == L and keep != list(range(L))
        assert checked > n // 2                            # the exclusions did change the lists


@pytest.mark.gpu
@pytest.mark.parametrize("d,K,C", [(32, 10, 200), (64, 70, 200), (32, 64, 65), (16, 130, 150)])
def test_materialised_path_exact(d, K, C):
    """Other widths, and K > 64 at a fused width: -inf in the score block, and the rows that end
    short (the top-K kernel leaves no usable index in their empty slots) leave as -1 / -inf.  K up to
    130 takes several rounds of that kernel's 63 entries.  Several row blocks."""
    n_u = 90
    U, P = _ints(d + K, n_u, C, d)
    lists = _lists(U @ P.T, K, K)
    rng = np.random.default_rng(K)
    users = rng.integers(0, n_u, 75)
    Ud, Pd, ud = U.to(DEV), P.to(DEV), torch.from_numpy(users).to(DEV)
    seen = metrics.SeenIndex(_edges(lists, 1), n_u, C)
    want = _reference(U, P, users, lists, K)
    assert bool((want[1] == -1).any())
    none = [[] for _ in lists]
    for kw in ({}, {"row_dtype": "bf16"}, {"batch_scores": 20 * C}):
        _same(recommend(Ud, Pd, K, users=ud, exclude=seen, **kw), want)
        _same(recommend(Ud, Pd, K, exclude=seen, **kw), _reference(U, P, None, lists, K))
        _same(recommend(Ud, Pd, K, users=ud, **kw), _reference(U, P, users, none, K))
        _same(recommend(Ud, Pd, K, **kw), _reference(U, P, None, none, K))
    _same(recommend(Ud.bfloat16(), Pd.bfloat16(), K, users=ud, exclude=seen), want)
    if d == 64:                                            # the same lists from the fused kernel
        f = recommend(Ud, Pd, 64, users=ud, exclude=seen)
        m = recommend(Ud, Pd, K, users=ud, exclude=seen)
        assert torch.equal(f[0], m[0][:, :64]) and torch.equal(f[1], m[1][:, :64])


@pytest.mark.gpu
def test_excluding_entry_is_graph_capturable():
    n_u, C, K, d = 200, 300, 10, 128
    U, P = _ints(2, n_u, C, d)
    lists = _lists(U @ P.T, K, 2)
    seen = metrics.SeenIndex(_edges(lists, 2), n_u, C)
    Ub, Pb = U.to(DEV).bfloat16(), P.to(DEV).bfloat16()
    topv = torch.zeros(n_u, K, device=DEV)
    topi = torch.zeros(n_u, K, dtype=torch.int32, device=DEV)
    lib = N.lib()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.check(lib.hgnn_score_topk_excl_bf16(
            N.ptr(Ub), None, n_u, N.ptr(Pb), C, d, K, N.ptr(seen.rowptr), N.ptr(seen.col), None,
            N.ptr(topv), N.ptr(topi), N.stream_ptr(DEV)), "hgnn_score_topk_excl_bf16")
    graph.replay()
    torch.cuda.synchronize()
    want = _reference(U, P, None, lists, K)
    assert torch.equal(topi.cpu().long(), want[1]) and torch.equal(topv.cpu(), want[0])
