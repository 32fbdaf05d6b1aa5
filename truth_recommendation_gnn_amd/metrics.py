"""Batched Recall@K / NDCG@K — the reference's ``evaluate`` (train_gnn.py:289-367) on device.

The reference loops over test users in Python: one [1,d]x[d,C] product, one ``torch.topk``, one
``sklearn.metrics.ndcg_score`` and several host syncs per user.  Here the grouping is a handful of
device sorts; then, for d in (64, 128), one fused kernel scores every test user against every
candidate on MFMA and keeps each user's top-(K+1) list without materialising the scores
(``hgnn_score_topk``), and a second one turns the lists into Recall/NDCG (``hgnn_topk_finish``).
The rare rows whose K-th score ties the next (sklearn's tie groups then need the whole row) and
other widths take the materialised path: one GEMM per user batch (torch.mm -> hipBLASLt) and
``hgnn_topk_metrics`` over it.  Same arguments, same return values.

``row_dtype="bf16"`` (or ``torch.bfloat16`` tables) ranks the rows rounded to bf16: the fused
kernel is then ``hgnn_score_topk_bf16`` (bf16 MFMA, fp32 accumulation, fp32 lists), everything
else runs as above on the fp32 widening of the rounded rows.  The default stays fp32.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _native as N
from . import ops


class _Grouped:
    """Test edges grouped per user: candidates, per-user unique relevant candidates, counts."""

    def __init__(self, test_edges: torch.Tensor, num_users: int, num_posts: int):
        te = test_edges.to(torch.int64)
        u, p_local = te[0], te[1] - num_users             # train_gnn.py:313-316
        if p_local.numel() and (int(p_local.min()) < 0 or int(p_local.max()) >= num_posts):
            raise ValueError("evaluate: test edge post id outside [num_users, num_users+num_posts)")
        if u.numel() and int(u.min()) < 0:
            raise ValueError("evaluate: negative user id in test_edges")
        # candidates: every post of the test set, sorted (train_gnn.py:320-322) — including the
        # posts of skipped (out-of-range) users, as in the reference
        self.cand, inv = torch.unique(p_local, sorted=True, return_inverse=True)
        C = int(self.cand.numel())
        keep = u < num_users                              # train_gnn.py:328
        u, c = u[keep], inv[keep]
        self.users, counts = torch.unique(u, sorted=True, return_counts=True)
        self.true_count = counts.to(torch.int32)
        key = torch.unique(u * max(C, 1) + c, sorted=True)     # (user, candidate) pairs, deduped
        ku = key // max(C, 1)
        per_user = torch.searchsorted(ku, self.users, right=True)
        self.rowptr = torch.cat([per_user.new_zeros(1), per_user]).to(torch.int32)
        self.true_cand = (key % max(C, 1)).to(torch.int32)


class _Default(str):
    """The ``row_dtype`` default: the string "fp32", told apart from a caller's own "fp32" by
    identity, so bf16 tables given with no ``row_dtype`` imply the bf16 path while an explicit
    "fp32" beside them is an error."""


_FP32 = _Default("fp32")


def _bf16_rows(user_emb: torch.Tensor, post_emb: torch.Tensor, row_dtype: str, what: str) -> bool:
    """Whether the call scores bf16 rows: ``row_dtype="bf16"``, or bf16 tables."""
    mode = ops._row_dtype_value(row_dtype, "row_dtype")
    dts = (user_emb.dtype, post_emb.dtype)
    if dts == (torch.bfloat16, torch.bfloat16):
        if mode == "fp32" and row_dtype is not _FP32:
            raise TypeError(f"{what}: bf16 embeddings with row_dtype='fp32'")
        return True
    if dts != (torch.float32, torch.float32):
        raise TypeError(f"{what}: fp32 embeddings (the reference dtype) or, for the bf16 rows, "
                        f"both tables in bf16 expected; got {dts[0]} and {dts[1]}")
    return mode == "bf16"


def _as_bf16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype == torch.bfloat16 else ops.rows_to_bf16(t)


def _fused_ok(d: int, fused: Optional[bool]) -> bool:
    if fused is None:
        return d in (64, 128)
    if fused and d not in (64, 128):
        raise ValueError(f"fused scoring supports d in (64, 128), got {d}")
    return fused


def _score_topk(U, rows, n, P, C, d, L, topv, topi, bf16, seen=None, excl_rows=None) -> None:
    """The fused kernel, hgnn_score_topk[_excl][_bf16]: the top-L list of output row r, which
    scores row ``rows[r]`` (or r) of U against P[:C], without the posts ``seen`` (a SeenIndex)
    lists for user ``excl_rows[r]`` (or r)."""
    entry = "hgnn_score_topk" + ("_excl" if seen is not None else "") + ("_bf16" if bf16 else "")
    excl = () if seen is None else (N.ptr(seen.rowptr), N.ptr(seen._col), N.ptr(excl_rows))
    N.check(getattr(N.lib(), entry)(N.ptr(U), N.ptr(rows), n, N.ptr(P), C, d, L, *excl,
                                    N.ptr(topv), N.ptr(topi), N.stream_ptr(topv.device)), entry)


def evaluate(test_edges: torch.Tensor, user_emb: torch.Tensor, post_emb: torch.Tensor,
             K: int = 10, num_users: Optional[int] = None,
             batch_scores: int = 1 << 30, fused: Optional[bool] = None,
             row_dtype: str = _FP32) -> Tuple[float, float]:
    """Mean Recall@K and NDCG@K over the test users (train_gnn.py:289-367).

    ``test_edges``: [2, E] user -> global post id (post ids offset by ``num_users``, as the
    reference builds them; ``num_users`` defaults to ``user_emb.shape[0]``, the reference's global).
    ``batch_scores`` bounds the floats of one materialised score matrix (rows x candidates).
    ``fused`` (default: when d is 64 or 128) scores and ranks in one kernel without materialising
    the scores (hgnn_score_topk); rows whose K-th score ties the next one are redone on the
    materialised path, which sklearn's tie groups need.
    ``row_dtype``: "fp32" (the default whatever ``ops.ROW_DTYPE`` says: the reference-parity
    path) or "bf16"; ``torch.bfloat16`` tables imply "bf16".  The bf16 mode rounds the rows that
    are scored (the test users' and the candidates') to bf16, R(T) = T.to(bfloat16).float(), and
    returns what the fp32 path returns on R(U), R(P): the fused kernel reads the bf16 rows
    themselves (hgnn_score_topk_bf16), the materialised path (tie redo, other widths) their fp32
    widening."""
    bf16 = _bf16_rows(user_emb, post_emb, row_dtype, "evaluate")
    dev = N.require_device(user_emb, post_emb, test_edges)
    nu = int(user_emb.shape[0]) if num_users is None else int(num_users)
    g = _Grouped(test_edges, nu, int(post_emb.shape[0]))
    n_rows, C = int(g.users.numel()), int(g.cand.numel())
    if n_rows == 0:
        return math.nan, math.nan                         # np.mean([]) in the reference
    d = int(user_emb.shape[1])
    ld = (C + 3) // 4 * 4                                  # 16-B aligned score rows
    P_c = post_emb.new_zeros(ld, d)                        # candidates, zero-padded to ld
    P_c[:C] = post_emb.index_select(0, g.cand)
    recall = torch.empty(n_rows, dtype=torch.float64, device=dev)
    ndcg = torch.empty(n_rows, dtype=torch.float64, device=dev)
    lib = N.lib()
    users32 = g.users.to(torch.int32)
    if bf16:
        # only the scored rows are cast: row r of U_b is test user r's, P_b the padded candidates
        U_b = _as_bf16(user_emb.index_select(0, g.users))
        P_b = _as_bf16(P_c)
        P_c = None                                         # the materialised path widens P_b
    if _fused_ok(d, fused):
        k = min(K, C)
        L = k + 1 if C > k else k
        topv = torch.empty(n_rows, L, dtype=torch.float32, device=dev)
        topi = torch.empty(n_rows, L, dtype=torch.int32, device=dev)
        tie = torch.empty(n_rows, dtype=torch.int32, device=dev)
        if bf16:
            _score_topk(U_b, None, n_rows, P_b, C, d, L, topv, topi, True)
        else:
            _score_topk(user_emb.contiguous(), users32, n_rows, P_c, C, d, L, topv, topi, False)
        N.check(lib.hgnn_topk_finish(N.ptr(topv), N.ptr(topi), n_rows, L, C, K, N.ptr(g.rowptr),
                                     N.ptr(g.true_cand), N.ptr(g.true_count), N.ptr(recall),
                                     N.ptr(ndcg), N.ptr(tie), N.stream_ptr(dev)),
                "hgnn_topk_finish")
        redo = torch.nonzero(tie).reshape(-1).to(torch.int32)   # one sync
        n_redo = int(redo.numel())
    else:
        redo, n_redo = None, n_rows                        # every row on the materialised path
    if n_redo:
        if bf16:
            P_c = P_b.float()
        rows = max(1, min(n_redo, batch_scores // ld))
        buf = torch.empty(rows, ld, dtype=torch.float32, device=dev)
        for r0 in range(0, n_redo, rows):
            r1 = min(n_redo, r0 + rows)
            S = buf[: r1 - r0]                             # columns >= C (padding) are ignored
            rmap = (torch.arange(r0, r1, dtype=torch.int32, device=dev) if redo is None
                    else redo[r0:r1])
            U_r = (U_b.index_select(0, rmap.long()).float() if bf16
                   else user_emb.index_select(0, users32[rmap.long()]))
            torch.mm(U_r, P_c.T, out=S)
            N.check(lib.hgnn_topk_metrics_rows(
                N.ptr(S), r1 - r0, C, ld, N.ptr(rmap), N.ptr(g.rowptr), N.ptr(g.true_cand),
                N.ptr(g.true_count), K, None, N.ptr(recall), N.ptr(ndcg), N.stream_ptr(dev)),
                "hgnn_topk_metrics_rows")
    return float(recall.mean()), float(ndcg.mean())


def topk_metrics(scores: torch.Tensor, true_rowptr: torch.Tensor, true_cand: torch.Tensor,
                 true_count: torch.Tensor, K: int = 10):
    """Raw kernel: per-row (topk_idx, recall, ndcg) of a [rows, C] score matrix."""
    dev = N.require_device(scores, true_rowptr, true_cand, true_count)
    n, C = scores.shape
    k = min(K, C)
    topk = torch.empty(n, k, dtype=torch.int32, device=dev)
    recall = torch.empty(n, dtype=torch.float64, device=dev)
    ndcg = torch.empty(n, dtype=torch.float64, device=dev)
    N.check(N.lib().hgnn_topk_metrics(
        N.ptr(scores), n, C, scores.stride(0), N.ptr(true_rowptr), N.ptr(true_cand),
        N.ptr(true_count), K, N.ptr(topk), N.ptr(recall), N.ptr(ndcg), N.stream_ptr(dev)),
        "hgnn_topk_metrics")
    return topk, recall, ndcg


class SeenIndex:
    """The posts each user has already engaged with, as ``recommend(..., exclude=)`` reads them:
    ``rowptr`` (int32 ``[num_users + 1]``) and ``col`` (int32, ascending and unique per user) on
    the device of ``edges``.  ``edges``: int ``[2, M]`` (user row, post index) pairs in any order,
    duplicates allowed: the training graph's ('user', 'engages', 'post') edge_index as it is.
    Build it once and reuse it for every call; the grouping is a device sort."""

    def __init__(self, edges: torch.Tensor, num_users: int, num_posts: int):
        dev = N.require_device(edges)
        if edges.dim() != 2 or edges.shape[0] != 2 or edges.is_floating_point() or \
                edges.is_complex() or edges.dtype == torch.bool:
            raise ValueError("SeenIndex: edges must be an integer [2, M] tensor")
        self.num_users, self.num_posts = int(num_users), int(num_posts)
        if self.num_users < 0 or self.num_posts < 0 or self.num_posts >= 2 ** 31 or \
                self.num_users >= 2 ** 31:
            raise ValueError("SeenIndex: num_users and num_posts must lie in [0, 2^31)")
        M = int(edges.shape[1])
        if M >= 2 ** 31:
            raise ValueError(f"SeenIndex: {M} edges; int32 row pointers hold fewer than 2^31")
        e = edges.to(torch.int64)
        u, p = e[0], e[1]
        if M:
            lo_u, hi_u, lo_p, hi_p = torch.stack([u.min(), u.max(), p.min(), p.max()]).tolist()
            if lo_u < 0 or hi_u >= self.num_users:
                raise ValueError(f"SeenIndex: user row outside [0, {self.num_users})")
            if lo_p < 0 or hi_p >= self.num_posts:
                raise ValueError(f"SeenIndex: post index outside [0, {self.num_posts})")
        key = torch.unique(u * max(self.num_posts, 1) + p, sorted=True)   # deduped, (user, post)
        per_user = torch.searchsorted(
            key, torch.arange(1, self.num_users + 1, device=dev) * max(self.num_posts, 1))
        self.rowptr = torch.cat([per_user.new_zeros(1), per_user]).to(torch.int32)
        # one spare element: an index without edges still has a col pointer to hand to the library
        self._col = torch.zeros(int(key.numel()) + 1, dtype=torch.int32, device=dev)
        self._col[:-1] = key % max(self.num_posts, 1)
        self.col = self._col[:-1]


def _check_users(users: torch.Tensor, n_u: int) -> torch.Tensor:
    if users.dim() != 1 or users.is_floating_point() or users.is_complex() or \
            users.dtype == torch.bool:
        raise ValueError("recommend: users must be a 1-D integer tensor of user_emb rows")
    if users.numel():
        lo, hi = torch.stack([users.min(), users.max()]).tolist()
        if lo < 0 or hi >= n_u:
            raise ValueError(f"recommend: users outside [0, {n_u})")
    return users.to(torch.int32).contiguous()


def _mask_seen(S: torch.Tensor, seen: SeenIndex, ids: torch.Tensor) -> None:
    """S[r, c] = -inf for every post c that user ids[r] (int64) has seen."""
    start = seen.rowptr[ids].long()
    count = seen.rowptr[ids + 1].long() - start
    total = int(count.sum())
    if total == 0:
        return
    r = torch.repeat_interleave(torch.arange(ids.numel(), device=S.device), count,
                                output_size=total)
    first = torch.cumsum(count, 0) - count                 # of each row, in the flattened lists
    c = seen.col[start[r] + (torch.arange(total, device=S.device) - first[r])].long()
    S[r, c] = -math.inf


def recommend(user_emb: torch.Tensor, post_emb: torch.Tensor, K: int = 10,
              batch_scores: int = 1 << 30, fused: Optional[bool] = None,
              row_dtype: str = _FP32, users: Optional[torch.Tensor] = None,
              exclude=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-K posts for every user row: ``(topk_scores, topk_indices)``, each ``[n_users, k]``,
    k = min(K, n_posts) — the scoring of ``recommend_for_user_inductive`` (inference.py:427-429:
    ``torch.topk(user_emb @ known_post_emb.T, min(K, len(scores)))``) for a whole batch of users
    at once.  Scores descend; equal scores list the lower post index first.  ``fused`` (default
    for d in (64, 128), K <= 64): one kernel, no score matrix.  ``row_dtype`` as in ``evaluate``:
    "bf16", or ``torch.bfloat16`` tables, ranks the rows rounded to bf16 (the fused kernel on
    bf16 MFMA; other widths and K > 64 on the materialised path over the widened rows), and the
    returned scores are fp32 scores of the rounded rows.

    ``users``: an int tensor ``[n]`` of ``user_emb`` rows (repeats and an empty tensor allowed);
    output row r is then for ``users[r]``.  ``exclude``: a ``SeenIndex`` (build it once), or an
    int ``[2, M]`` tensor of (user row, post index) pairs from which one is built for the call:
    the posts a user has already engaged with never appear in that user's list.  It is keyed by
    the row of ``user_emb``, not by the position in ``users``.  The fused kernels test the
    exclusion themselves (hgnn_score_topk_excl, hgnn_score_topk_excl_bf16); the materialised path
    writes -inf into the scores.  A user with fewer than k posts left gets score -inf and index
    -1 in the empty slots.  With ``row_dtype="bf16"`` on fp32 tables only the selected users'
    rows are cast.

    The materialised path ranks in rounds of 63 (hgnn_topk_metrics' list), so K > 63 there
    returns the lists whether or not ``users`` / ``exclude`` are given."""
    bf16 = _bf16_rows(user_emb, post_emb, row_dtype, "recommend")
    seen = exclude if isinstance(exclude, SeenIndex) or exclude is None else None
    dev = N.require_device(user_emb, post_emb, users, seen.rowptr if seen is not None else exclude)
    n_u, C = int(user_emb.shape[0]), int(post_emb.shape[0])
    if C == 0:
        raise ValueError("recommend: no posts to rank")
    if exclude is not None and seen is None:
        seen = SeenIndex(exclude, n_u, C)
    if seen is not None and (seen.num_users, seen.num_posts) != (n_u, C):
        raise ValueError(f"recommend: exclude was built for {seen.num_users} users x "
                         f"{seen.num_posts} posts, the tables hold {n_u} x {C}")
    users32 = None if users is None else _check_users(users, n_u)
    n = n_u if users is None else int(users32.numel())
    k = min(K, C)
    d = int(user_emb.shape[1])
    out_s = torch.empty(n, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(n, k, dtype=torch.int32, device=dev)
    if n == 0:
        return out_s, out_i.long()
    if bf16 and user_emb.dtype != torch.bfloat16:          # row_dtype="bf16" on fp32 tables
        # only the selected rows are cast: row r of U is users[r]'s
        U = ops.rows_to_bf16(user_emb if users is None else user_emb.index_select(0, users32))
        rows = None
    else:
        U, rows = user_emb.contiguous(), users32
    P = _as_bf16(post_emb) if bf16 else post_emb.contiguous()
    if _fused_ok(d, fused) and k <= 64:
        _score_topk(U, rows, n, P, C, d, k, out_s, out_i, bf16, seen, users32)
        return out_s, out_i.long()
    # materialised: the scores of a block of rows, -inf at the excluded posts, then the K best in
    # rounds of up to 63 (hgnn_topk_metrics' list) with each round's winners set to -inf.  That
    # kernel never lists a -inf score, and what it leaves in the slots past a row's last real
    # entry is not an index to read with (INT_MAX, or a padding position of its scan): the slots
    # that hold an entry are counted from the scores instead, and the empty ones point at a
    # padding column of -inf.  Without exclusions no row ends short (k <= C) and none of that runs.
    ld = (C + (3 if seen is None else 4)) // 4 * 4         # 16-B rows (and that padding column)
    P_c = torch.zeros(ld, d, dtype=torch.float32, device=dev)
    P_c[:C] = P.float()
    nb = max(1, min(n, batch_scores // ld))
    buf = torch.empty(nb, ld, dtype=torch.float32, device=dev)
    no_rel = torch.zeros(nb + 1, dtype=torch.int32, device=dev)   # empty relevance sets
    scratch = torch.empty(2, nb, dtype=torch.float64, device=dev)
    lib = N.lib()
    for r0 in range(0, n, nb):
        r1 = min(n, r0 + nb)
        S = buf[: r1 - r0]
        U_r = U[r0:r1] if rows is None else U.index_select(0, rows[r0:r1])
        torch.mm(U_r.float(), P_c.T, out=S)
        if seen is not None:
            _mask_seen(S, seen, (torch.arange(r0, r1, device=dev) if users32 is None
                                 else users32[r0:r1].long()))
            S[:, C:] = -math.inf
        for k0 in range(0, k, 63):
            kr = min(63, k - k0)
            idx = torch.empty(r1 - r0, kr, dtype=torch.int32, device=dev)
            N.check(lib.hgnn_topk_metrics(
                N.ptr(S), r1 - r0, C, ld, N.ptr(no_rel), N.ptr(no_rel), N.ptr(no_rel), kr,
                N.ptr(idx), N.ptr(scratch[0]), N.ptr(scratch[1]), N.stream_ptr(dev)),
                "hgnn_topk_metrics")
            at = idx.long()
            if seen is not None:
                left = (S[:, :C] > -math.inf).sum(1, keepdim=True)   # candidates still unlisted
                empty = torch.arange(kr, device=dev) >= left
                at.masked_fill_(empty, ld - 1)
                idx.masked_fill_(empty, -1)
            out_s[r0:r1, k0:k0 + kr] = S.gather(1, at)
            out_i[r0:r1, k0:k0 + kr] = idx
            if k0 + kr < k:
                S.scatter_(1, at, -math.inf)
    return out_s, out_i.long()
