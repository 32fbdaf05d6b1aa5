"""The BCE link loss at saturated scores, against a float64 evaluation of the formula.

Every other test of the fused loss draws its tables as ``0.3 * randn`` (scores within a few units
of 0) and scales its tolerance by the largest entry of the whole gradient, so none of them sees a
coefficient or a loss term of a saturated pair, which is what a trained model produces.  Here every
pair's score is known exactly, rows of dU and dP are pure in magnitude, and the criterion is
elementwise and relative to the row's own terms.

**Inputs.**  Users and posts belong to one *level* z_L each; all of a level's pairs score inside
[z_L, 2 z_L] (``LEVELS``; ``EXTREME`` holds z = 100 and z = 1e4, checked on their own).  A user row
has at most four non-zero entries, small integers that sum to 4; a post row is ``s_L * b`` with
integers b in [b0, b1] in every column, negated for a post of the negative side, where s_L is a
power of two with ``4 b0 s_L >= z_L`` and ``4 b1 s_L <= 2 z_L`` (a kind's first post keeps to the
lowest quarter of that range, so that every level has pairs next to z_L itself).  Every entry has
at most 8 significant bits, so the tables are exact as bf16 rows and every dot product is exact in
fp32 in any order.  (Level 0: the users' and the posts' non-zeros sit in different columns.)  A level has
two groups of users: *right* (positives score +z, negatives -z: small coefficients and loss terms)
and *wrong* (the opposite), and four kinds of posts, each touched by one kind of pair only:
positives of the right users, positives of the wrong ones, negatives of the right ones, negatives
of the wrong ones.  So every row of dU and dP has the magnitude of one level's coefficients on one
side.  Degrees cover 1, 63, 64 and 65 (the kernels walk 64 positions at a time).

**Reference** (``reference``): float64 numpy with log1p, per pair
``w softplus(-+z)``, ``-g c w sigmoid(-z) / E`` for a positive, ``g sigmoid(z) / (E k)`` for a
negative; dU and dP are the coefficient-weighted sums of the (exact) rows, and beside each element
``A = sum |coefficient| |entry|``.

**Criterion for the gradients**: elementwise ``|got - ref| <= eps * A + floor`` with
``eps = (2 zmax_row + 8 + n_terms) 2^-24``: 2 |z| for the rounding of ``z log2(e)`` ahead of the
hardware exp, 8 for exp, rcp, 1 + t and the scale products at 1-2 ulp each, n_terms for the fp32
accumulation.  ``floor = 2 n_terms 2^-126 max(1, |entry|) max(1, g)`` is what fp32 itself cannot
hold: below 2^-126 an exponential, a coefficient or a product may be flushed to 0 (or rounded as a
subnormal), once where the coefficient is formed and once where it is accumulated.  It matters
from level 60 up only, whose right-side coefficients reach e^-120; at level 30 the smallest
coefficient is still 1e6 times the floor.  ``test_fp32_restatement_*`` run an fp32 torch
restatement of the kernels' forms through the same check on the CPU: the bound is reachable by
fp32 arithmetic on these inputs, and the forms the kernels had before (``1/(1+t) - 1``,
``log(1 + t)``) miss it from level 8 up.

**Criterion for the loss**: on the subgraph of the right-side users of the levels >= 12 (the whole
loss is made of small terms) the loss is checked relative to the float64 loss; the yardstick is
fp32 ``torch.nn.functional.softplus`` on the CPU (log1p) on the same scores, its worst relative
error over the terms that are normal fp32 numbers (a term below 2^-126 has no relative precision in
fp32, and those terms together are asserted to be below 2^-60 of the loss); the kernels may have 16
times that.  On the full graph the loss is checked to 1e-5 of itself (its large terms dominate:
at most 65 + 16 fp32 additions of 2^-24 each).

Measured figures (largest ``err / bound`` per case, the yardstick and the kernels' loss error) are
printed as ``SATURATION {json}`` lines; ``profiles/loss_saturation.jsonl`` keeps a run's."""
import functools
import json
import math
import pathlib
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from truth_recommendation_gnn_amd import minibatch, ops

ROOT = pathlib.Path(__file__).resolve().parents[1]
DEV = "cuda:0"
LEVELS = (0.0, 0.5, 2.0, 4.0, 8.0, 10.0, 12.0, 14.0, 16.0, 16.5, 17.0, 20.0, 30.0, 60.0, 80.0)
EXTREME = (100.0, 1.0e4)
RIGHT_FROM = 12.0                  # the all-right-side subgraph: the levels from here up
DEGREES = (1, 63, 64, 65)
EXTRA_DEGREES = (2, 5, 9)          # each group's second user
PATTERNS = ((1, 1, 1, 1), (2, 1, 1), (2, 2), (3, 1), (4,))    # a user's non-zeros: they sum to 4
KMAX = 3
UP = 2.5                           # the upstream gradient of every backward here
U24 = 2.0 ** -24
TINY = 2.0 ** -126
LOSS_MARGIN = 16.0
KINDS = ("pos_right", "pos_wrong", "neg_right", "neg_wrong")


# ----------------------------------------------------------------------------- inputs
def level_scale(z):
    """(s, b0, b1) of a level: post entries are s * b, b0 <= b <= b1."""
    if z == 0.0:
        return 1.0, 8, 16
    s = 2.0 ** math.floor(math.log2(z / 32.0))
    return s, math.ceil(z / (4 * s)), math.floor(2 * z / (4 * s))


@functools.lru_cache(maxsize=None)
def graph(d, which="full"):
    """The tables, edges, negatives and weights of one width, on the CPU.  ``which``: "full" (all
    ``LEVELS``, both groups), "right" (the right-side users of the levels >= ``RIGHT_FROM``) or
    "extreme" (``EXTREME``, both groups)."""
    levels = {"full": LEVELS, "extreme": EXTREME,
              "right": tuple(z for z in LEVELS if z >= RIGHT_FROM)}[which]
    groups = ("right",) if which == "right" else ("right", "wrong")
    rng = np.random.default_rng(1000 + d + {"full": 0, "right": 1, "extreme": 2}[which])
    U, P = [], []
    ulevel, uright, plevel, pkind = [], [], [], []
    eu, ep, en = [], [], []
    for li, z in enumerate(levels):
        s, b0, b1 = level_scale(z)
        ucols = np.arange(0, d // 2) if z == 0.0 else np.arange(d)
        pcols = np.arange(d // 2, d) if z == 0.0 else np.arange(d)
        for gi, grp in enumerate(groups):
            right = grp == "right"
            n_per_kind = 1 if li % 4 == 0 else 2      # one post per kind: a post of 66+ positives
            ids = {}
            for kind, sign in (("pos", 1.0 if right else -1.0), ("neg", -1.0 if right else 1.0)):
                ids[kind] = []
                for j in range(n_per_kind):
                    # a kind's first post scores in the band's lowest quarter (a sum of four
                    # uniform entries would sit mid-band: level 60 would be level 90), its second
                    # post anywhere in the band
                    hi = b0 + max(1, (b1 - b0) // 4) if j == 0 else b1
                    row = np.zeros(d)
                    row[pcols] = sign * s * rng.integers(b0, hi + 1, pcols.size)
                    ids[kind].append(len(P))
                    P.append(row)
                    plevel.append(z)
                    pkind.append(KINDS.index(f"{kind}_{grp}"))
            prob = [1.0] if n_per_kind == 1 else [0.75, 0.25]
            n = li * len(groups) + gi
            # (the rotation gives both sides a post of more than 64 positives)
            for deg in (DEGREES[(n + li // 4) % 4], EXTRA_DEGREES[n % 3]):
                pats = [p for p in PATTERNS if len(p) <= ucols.size]
                pat = pats[int(rng.integers(len(pats)))]
                row = np.zeros(d)
                row[rng.choice(ucols, len(pat), replace=False)] = pat
                u = len(U)
                U.append(row)
                ulevel.append(z)
                uright.append(right)
                eu.append(np.full(deg, u))
                ep.append(rng.choice(ids["pos"], deg, p=prob))
                en.append(rng.choice(ids["neg"], (deg, KMAX), p=prob))
    U, P = np.array(U), np.array(P)
    eu, ep, en = np.concatenate(eu), np.concatenate(ep), np.concatenate(en)
    # ids and the COO order shuffled: the levels interleave in every block of four users
    uperm, pperm, eperm = (rng.permutation(n) for n in (len(U), len(P), eu.size))
    Us, Ps = np.empty_like(U), np.empty_like(P)
    Us[uperm], Ps[pperm] = U, P
    inv_u, inv_p = np.empty(len(U), int), np.empty(len(P), int)
    inv_u[uperm], inv_p[pperm] = np.arange(len(U)), np.arange(len(P))
    eu, ep, en = uperm[eu][eperm], pperm[ep][eperm], pperm[en][eperm]
    E = eu.size
    g = types.SimpleNamespace(
        d=d, which=which, U=Us, P=Ps, E=E, nu=len(U), np_=len(P), u=eu, p=ep,
        neg={1: en[:, 0].copy(), KMAX: en.copy()},
        ulevel=np.array(ulevel)[inv_u], uright=np.array(uright)[inv_u],
        plevel=np.array(plevel)[inv_p], pkind=np.array(pkind)[inv_p],
        # dyadic per-edge weights: every product with them is exact
        w_edge=np.array([0.5, 1.0, 2.0, 0.75, 1.5])[np.arange(E) % 5],
        w_mean=np.full(E, 1.25), refs={})
    g.entry_max = float(max(np.abs(Us).max(), np.abs(Ps).max()))
    return g


def softplus64(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid64(x):
    t = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def scores(g, k):
    """Every pair's exact score: the positives' [E] and the negatives' [E, k]."""
    neg = g.neg[k].reshape(g.E, k)
    zp = (g.U[g.u] * g.P[g.p]).sum(1)
    zn = (g.U[g.u][:, None, :] * g.P[neg]).sum(-1)
    return zp, zn, neg


def reference(g, k, weighting, c, up):
    """The float64 loss and gradients of one (k, weighting, cscale, upstream gradient); computed
    once and never changed.  Per row of dU / dP also A, S (A with every sigmoid replaced by 1: the
    row's scale), the largest |z| and the number of terms."""
    key = (k, weighting, float(c), float(up))
    if key in g.refs:
        return g.refs[key]
    w = g.w_edge if weighting == "edge" else np.ones(g.E)
    E = g.E
    zp, zn, neg = scores(g, k)
    loss = (c * w * softplus64(-zp)).sum() / E + softplus64(zn).sum() / (E * k)
    sp, sn = up * c * w / E, np.full(zn.shape, up / (E * k))       # the pairs' scales
    cp, cn = -sp * sigmoid64(-zp), sn * sigmoid64(zn)
    un, nn = np.repeat(g.u, k), neg.reshape(-1)
    cn, sn, znf = cn.reshape(-1), sn.reshape(-1), zn.reshape(-1)
    r = types.SimpleNamespace(loss=float(loss), zp=zp, zn=zn)
    for name, rows, n, i_p, i_n, other, o_p, o_n in (("dU", g.nu, g.nu, g.u, un, g.P, g.p, nn),
                                                     ("dP", g.np_, g.np_, g.p, nn, g.U, g.u, un)):
        val, A, S = (np.zeros((n, g.d)) for _ in range(3))
        np.add.at(val, i_p, cp[:, None] * other[o_p])
        np.add.at(val, i_n, cn[:, None] * other[o_n])
        np.add.at(A, i_p, np.abs(cp)[:, None] * np.abs(other[o_p]))
        np.add.at(A, i_n, np.abs(cn)[:, None] * np.abs(other[o_n]))
        np.add.at(S, i_p, sp[:, None] * np.abs(other[o_p]))
        np.add.at(S, i_n, sn[:, None] * np.abs(other[o_n]))
        zmax, nt = np.zeros(n), np.zeros(n)
        np.maximum.at(zmax, i_p, np.abs(zp))
        np.maximum.at(zmax, i_n, np.abs(znf))
        np.add.at(nt, i_p, 1.0)
        np.add.at(nt, i_n, 1.0)
        setattr(r, name, types.SimpleNamespace(val=val, A=A, S=S, zmax=zmax, nt=nt))
    g.refs[key] = r
    return r


# ----------------------------------------------------------------------------- criteria
def grad_ratio(got, ref, g, up, with_z=True):
    """``|got - ref| / (eps A + floor)`` per element (0 where both are 0, inf where only the
    bound is)."""
    got = np.asarray(got.detach().double().cpu().numpy() if torch.is_tensor(got) else got)
    eps = ((2.0 * ref.zmax if with_z else 0.0) + 8.0 + ref.nt) * U24
    floor = 2.0 * ref.nt * TINY * max(1.0, g.entry_max) * max(1.0, up)
    bound = eps[:, None] * ref.A + floor[:, None]
    err = np.abs(got - ref.val)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / bound)


def by_level(g, ratio_u, ratio_p):
    """The largest ratio per (level, side) over the rows of dU and of dP."""
    out = {}
    for z in sorted(set(g.ulevel)):
        for right in (True, False):
            rows_u = (g.ulevel == z) & (g.uright == right)
            rows_p = (g.plevel == z) & (np.isin(g.pkind, (0, 2)) == right)
            if rows_u.any():
                out[(z, "right" if right else "wrong")] = (
                    float(ratio_u[rows_u].max()), float(ratio_p[rows_p].max()))
    return out


def failing(levels):
    return sorted({float(z) for (z, _), (a, b) in levels.items() if max(a, b) > 1.0})


def check_grads(tag, g, got_dU, got_dP, ref, up):
    """Assert the gradient criterion on the full graph; returns the figures."""
    assert bool(torch.isfinite(got_dU).all()) and bool(torch.isfinite(got_dP).all()), tag
    levels = by_level(g, grad_ratio(got_dU, ref.dU, g, up), grad_ratio(got_dP, ref.dP, g, up))
    worst_u = max(a for a, _ in levels.values())
    worst_p = max(b for _, b in levels.values())
    fig = {"case": tag, "worst_dU": worst_u, "worst_dP": worst_p, "failing_levels": failing(levels)}
    print("SATURATION", json.dumps(fig))
    for (z, side), (a, b) in sorted(levels.items()):
        print(f"  {tag}: level {z:g} {side}: dU {a:.3g} dP {b:.3g} of the bound")
    assert not fig["failing_levels"], (
        f"{tag}: rows beyond eps * A at the levels {fig['failing_levels']} "
        f"(worst dU {worst_u:.3g}, dP {worst_p:.3g} of the bound)")
    return fig


def yardstick(g, k):
    """fp32 ``softplus`` (log1p) on the CPU on the pairs' scores against float64: the worst relative
    error over the terms that are normal fp32 numbers."""
    zp, zn, _ = scores(g, k)
    x = np.concatenate([-zp, zn.reshape(-1)])
    want = softplus64(x)
    got = torch.nn.functional.softplus(torch.from_numpy(x).float()).double().numpy()
    assert np.array_equal(torch.from_numpy(x).float().double().numpy(), x)     # exact in fp32
    normal = want >= TINY
    assert normal.sum() >= x.size // 2 and want[~normal].sum() <= 2.0 ** -60 * want.sum()
    return float((np.abs(got - want)[normal] / want[normal]).max())


def check_small_loss(tag, g, k, got_loss, ref):
    yard = yardstick(g, k)
    rel = abs(float(got_loss) - ref.loss) / ref.loss
    fig = {"case": tag, "loss": float(got_loss), "loss_f64": ref.loss, "loss_rel_err": rel,
           "yardstick_rel_err": yard, "allowed": LOSS_MARGIN * yard}
    print("SATURATION", json.dumps(fig))
    assert 0.0 < yard < 1e-6, yard
    assert rel <= LOSS_MARGIN * yard, (
        f"{tag}: the all-right-side loss {float(got_loss)!r} is {rel:.3g} off the float64 "
        f"{ref.loss!r}; fp32 softplus is {yard:.3g} off at worst ({LOSS_MARGIN:g} x allowed)")
    return fig


def check_extreme(tag, g, got_loss, got_dU, got_dP, ref, up):
    """z = 100 and z = 1e4: finite; the wrong side's loss terms are |z| and its coefficients the
    scale itself, to fp32 rounding (t is 0 or a subnormal there: no exp error to allow for); a
    right-side coefficient is at most 2^-126 of its scale."""
    for t in (got_loss, got_dU, got_dP):
        assert bool(torch.isfinite(t).all()), tag
    figs = {"case": tag}
    for name, got, rr, right in (("dU", got_dU, ref.dU, g.uright),
                                 ("dP", got_dP, ref.dP, np.isin(g.pkind, (0, 2)))):
        ratio = grad_ratio(got, rr, g, up, with_z=False)
        figs[f"wrong_{name}"] = float(ratio[~right].max())
        gotn = got.detach().double().cpu().numpy()
        small = np.abs(gotn[right]) / np.maximum(TINY * rr.S[right], 1e-300)
        figs[f"right_{name}_of_2^-126_scale"] = float(small.max())
        assert float(np.abs(rr.val[right]).max()) < TINY * float(rr.S[right].max())
    # the loss: the wrong side's terms are |z| exactly; per lane at most 65 + 16 fp32 additions
    figs["loss_rel_err"] = abs(float(got_loss) - ref.loss) / ref.loss
    print("SATURATION", json.dumps(figs))
    assert figs["wrong_dU"] <= 1.0 and figs["wrong_dP"] <= 1.0, figs
    assert figs["right_dU_of_2^-126_scale"] <= 1.0 and figs["right_dP_of_2^-126_scale"] <= 1.0, figs
    assert figs["loss_rel_err"] <= (max(DEGREES) + 16) * U24, figs
    return figs


# ----------------------------------------------------------------------------- fp32 on the CPU
def fp32_restatement(g, k, weighting, c, up, stable=True):
    """The kernels' arithmetic in fp32 torch on the CPU: t = exp(-|z|), the coefficients from it,
    the scale products in the kernels' order, fp32 sums.  ``stable=False``: the forms the kernels
    had before (``1/(1+t) - 1``, ``log(1 + t)``)."""
    f32 = torch.float32
    U, P = torch.from_numpy(g.U).to(f32), torch.from_numpy(g.P).to(f32)
    u, p = torch.from_numpy(g.u), torch.from_numpy(g.p)
    neg = torch.from_numpy(g.neg[k].reshape(g.E, k))
    w = torch.from_numpy(g.w_edge if weighting == "edge" else np.ones(g.E)).to(f32)
    zp = (U[u] * P[p]).sum(1)
    zn = (U[u][:, None, :] * P[neg]).sum(-1).reshape(-1)
    inv_e = torch.tensor(1.0 / (g.E * k), dtype=f32)
    ck = torch.tensor(c, dtype=f32) * float(k)
    one = torch.ones((), dtype=f32)

    def sig(x, t):
        r = one / (one + t)
        return torch.where(x >= 0, r, t * r)

    def log1p_t(t):
        uu = one + t
        dd = uu - one
        return torch.where(dd == 0, t, torch.log(uu) * (t / torch.where(dd == 0, one, dd)))

    tp, tn = torch.exp(-zp.abs()), torch.exp(-zn.abs())
    coef = -sig(-zp, tp) if stable else sig(zp, tp) - one
    hp = (ck * inv_e * coef * w) * torch.tensor(up, dtype=f32)
    hn = (inv_e * sig(zn, tn)) * torch.tensor(up, dtype=f32)
    un, nn = u.repeat_interleave(k), neg.reshape(-1)
    dU = torch.zeros(g.nu, g.d, dtype=f32)
    dU.index_add_(0, u, hp[:, None] * P[p])
    dU.index_add_(0, un, hn[:, None] * P[nn])
    dP = torch.zeros(g.np_, g.d, dtype=f32)
    dP.index_add_(0, p, hp[:, None] * U[u])
    dP.index_add_(0, nn, hn[:, None] * U[un])
    lg = log1p_t if stable else (lambda t: torch.log(one + t))
    lpos = (w * (torch.clamp(-zp, min=0) + lg(tp))).sum()
    lneg = (torch.clamp(zn, min=0) + lg(tn)).sum()
    loss = float(ck.double() * inv_e.double() * lpos.double() + inv_e.double() * lneg.double())
    return loss, dU, dP


# ----------------------------------------------------------------------------- CPU
def test_graph_is_what_the_docstring_says():
    for d in (64, 128, 16, 5):
        for which in ("full", "right", "extreme"):
            g = graph(d, which)
            for t in (g.U, g.P):      # exact as bf16 rows
                tt = torch.from_numpy(t).float()
                assert torch.equal(tt.bfloat16().float(), tt) and bool((tt.double() == tt).all())
            assert (g.U >= 0).all() and (g.U == 0).mean() > 0.15
            zp, zn, neg = scores(g, KMAX)
            ul = g.ulevel[g.u]
            sign = np.where(g.uright[g.u], 1.0, -1.0)
            assert (zp * sign >= ul).all() and (zp * sign <= 2 * ul).all()
            assert (-zn * sign[:, None] >= ul[:, None]).all()
            assert (-zn * sign[:, None] <= 2 * ul[:, None]).all()
            # a post is touched by its own level's pairs of one kind only
            assert (g.plevel[g.p] == ul).all() and (g.plevel[neg] == ul[:, None]).all()
            assert (g.pkind[g.p] == np.where(g.uright[g.u], 0, 1)).all()
            assert (g.pkind[neg] == np.where(g.uright[g.u], 2, 3)[:, None]).all()
            deg = np.bincount(g.u, minlength=g.nu)
            assert set(DEGREES) <= set(deg.tolist()) and deg.min() >= 1
            if which == "full":
                assert sorted(set(g.ulevel)) == list(LEVELS) and 1000 < g.E < 2500
                assert np.bincount(g.p, minlength=g.np_).max() > 64
            if which == "right":
                assert g.uright.all() and g.ulevel.min() == RIGHT_FROM
            if which == "extreme":
                assert sorted(set(g.ulevel)) == list(EXTREME)
                z4 = np.abs(zp[ul == 1.0e4])
                assert z4.min() >= 1.0e4 and z4.max() <= 2.0e4


@pytest.mark.parametrize("k,weighting,c", ((1, "mean", 1.25), (3, "edge", 1.0), (3, "mean", 1.25)))
@pytest.mark.parametrize("d", (64, 5))
def test_fp32_restatement_of_the_stable_forms_meets_the_bound(d, k, weighting, c):
    """The bound is reachable by fp32 arithmetic on these inputs: gradients on the full graph, the
    small loss on the all-right-side subgraph, the extreme levels."""
    g, tag = graph(d), f"cpu_fp32_d{d}_k{k}_{weighting}"
    loss, dU, dP = fp32_restatement(g, k, weighting, c, UP)
    ref = reference(g, k, weighting, c, UP)
    check_grads(tag, g, dU, dP, ref, UP)
    assert abs(loss - ref.loss) <= 1e-5 * ref.loss
    gr = graph(d, "right")
    loss, _, _ = fp32_restatement(gr, k, weighting, c, UP)
    check_small_loss(tag, gr, k, loss, reference(gr, k, weighting, c, UP))
    gx = graph(d, "extreme")
    loss, dU, dP = fp32_restatement(gx, k, weighting, c, UP)
    check_extreme(tag, gx, torch.tensor(loss), dU, dP, reference(gx, k, weighting, c, UP), UP)


def test_fp32_restatement_of_the_replaced_forms_misses_the_bound_from_level_8():
    """``1/(1+t) - 1`` and ``log(1 + t)`` through the same checks: the right-side rows are beyond
    the bound at every level from 8 up, the wrong-side rows and the lower levels are not, and the
    small loss is far outside its margin.  So the checks tell the two spellings apart."""
    g = graph(64)
    for k, weighting, c in ((1, "mean", 1.25), (3, "edge", 1.0)):
        _, dU, dP = fp32_restatement(g, k, weighting, c, UP, stable=False)
        ref = reference(g, k, weighting, c, UP)
        levels = by_level(g, grad_ratio(dU, ref.dU, g, UP), grad_ratio(dP, ref.dP, g, UP))
        print(k, weighting, "the replaced forms fail at the levels", failing(levels))
        # (level 80's right side is e^-80 / E and less: at or below 2^-126, inside the floor)
        assert set(failing(levels)) >= {z for z in LEVELS if 8.0 <= z <= 60.0}, failing(levels)
        assert min(failing(levels)) >= 2.0       # (between 2 and 8 the cancellation costs 1-5 ulp)
        assert all(max(v) <= 1.0 for (z, side), v in levels.items() if side == "wrong")
        # from level 17 up the right-side positives push nothing at all
        zero = dP[torch.from_numpy((g.plevel >= 17.0) & (g.pkind == 0))]
        assert zero.numel() > 0 and float(zero.abs().max()) == 0.0
        gr = graph(64, "right")
        loss, _, _ = fp32_restatement(gr, k, weighting, c, UP, stable=False)
        rr = reference(gr, k, weighting, c, UP)
        assert abs(loss - rr.loss) / rr.loss > 100 * LOSS_MARGIN * yardstick(gr, k)


def test_host_check_of_the_bce_terms_under_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "bce_terms_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "truth_recommendation_gnn_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "bce_terms_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bce_terms_check ok" in r.stdout


# ----------------------------------------------------------------------------- GPU
# One chosen case per line: (id, options).  d, k, weighting, rows ("fp32" / "bf16"), neg ("i64":
# int64 in COO order; "i32": int32 in the user-grouped order; "skewed": SkewedNegatives, the
# planned gather; "presorted"), zpack (HGNN_ZPACK=1), logq (a table of zeros through the LQ
# kernels, beside the call without one), api ("loss": ops.edge_bce_loss; "raw":
# ops.edge_bce_loss_raw; "blocks": raw with the dP gather in row blocks; "linkloss":
# minibatch.LinkLoss on one staged batch).
def _case(d=64, k=1, weighting="mean", rows="fp32", neg="i64", zpack=False, logq=False,
          api="loss"):
    return dict(d=d, k=k, weighting=weighting, rows=rows, neg=neg, zpack=zpack, logq=logq, api=api)


CASES = [
    ("d64_k1", _case()),
    ("d64_k3", _case(k=3)),
    ("d128_k1_edge_i32", _case(d=128, weighting="edge", neg="i32")),
    ("d128_k3_edge_bf16_skewed", _case(d=128, k=3, weighting="edge", rows="bf16", neg="skewed")),
    ("d64_k1_bf16", _case(rows="bf16")),
    ("d16_k1", _case(d=16, neg="i32")),
    ("d16_k3_edge_bf16", _case(d=16, k=3, weighting="edge", rows="bf16")),
    ("d5_k1_edge", _case(d=5, weighting="edge")),
    ("d5_k3_skewed", _case(d=5, k=3, neg="skewed")),
    ("d64_k1_skewed", _case(neg="skewed")),
    ("d64_k3_edge_presorted", _case(k=3, weighting="edge", neg="presorted")),
    ("d64_k1_zpack", _case(zpack=True)),
    ("d128_k3_edge_zpack_skewed", _case(d=128, k=3, weighting="edge", zpack=True, neg="skewed")),
    ("d64_k1_logq0", _case(logq=True)),
    ("d128_k3_edge_bf16_logq0", _case(d=128, k=3, weighting="edge", rows="bf16", logq=True)),
    ("d64_k1_zpack_skewed_logq0", _case(zpack=True, neg="skewed", logq=True)),
    ("d64_k1_raw", _case(api="raw")),
    ("d64_k3_edge_bf16_raw", _case(k=3, weighting="edge", rows="bf16", api="raw")),
    ("d64_k1_raw_row_blocks", _case(api="blocks", neg="i32")),
    ("d64_k1_linkloss", _case(api="linkloss")),
    ("d64_k3_linkloss", _case(k=3, api="linkloss")),
    ("d128_k1_edge_linkloss", _case(d=128, weighting="edge", api="linkloss")),
]


_DEV = {}


def _device(g):
    """The device copies of one graph: built once."""
    key = (g.d, g.which)
    if key not in _DEV:
        dev = torch.device(DEV)
        ei = torch.from_numpy(np.stack([g.u, g.p])).to(dev)
        csr = ops.relation_csr_for_loss(ei, g.nu, g.np_)
        perm_u = csr.bwd.perm.long()          # user-grouped position -> COO edge
        neg = {k: torch.from_numpy(v).to(dev) for k, v in g.neg.items()}
        w_mean = torch.from_numpy(g.w_mean).float().to(dev)
        _DEV[key] = types.SimpleNamespace(
            dev=dev, ei=ei, U=torch.from_numpy(g.U).float().to(dev),
            P=torch.from_numpy(g.P).float().to(dev), neg=neg,
            neg_user={k: v[perm_u].to(torch.int32).contiguous() for k, v in neg.items()},
            w_mean=w_mean, w_edge=torch.from_numpy(g.w_edge).float().to(dev),
            # the scalar the kernels get for weighting="mean": the device's fp32 mean, as it is
            c_mean=float(w_mean.mean()), chunk=csr.fwd.plan.chunk, n_heavy=csr.fwd.plan.n_heavy)
    return _DEV[key]


def _run(g, o, logq=None):
    """(loss, dU, dP, cscale, upstream gradient) of one case's path on graph ``g``."""
    t = _device(g)
    k, edge = o["k"], o["weighting"] == "edge"
    w = t.w_edge if edge else t.w_mean
    c = 1.0 if edge else t.c_mean
    if o["neg"] in ("i32", "skewed", "presorted"):
        neg, order = t.neg_user[k], "user"
        if o["neg"] != "i32":
            neg = ops.SkewedNegatives(neg) if o["neg"] == "skewed" else neg
    else:
        neg, order = t.neg[k], "edge"
    extra = {} if logq is None else {"logq": logq}
    if o["neg"] == "presorted":
        extra["presorted"] = ops.presort_negatives(g.nu, g.np_, t.ei, neg, order)
    if o["api"] == "linkloss":
        ll = minibatch.LinkLoss(g.E, g.nu, g.np_, t.dev, num_neg=k, weighting=o["weighting"])
        ll.load(t.ei[0].to(torch.int32), t.ei[1].to(torch.int32), t.neg[k].to(torch.int32),
                t.w_edge if edge else None)
        U, P = t.U.clone().requires_grad_(), t.P.clone().requires_grad_()
        loss = ll({"user": U, "post": P})
        (loss * UP).backward()
        return loss.detach(), U.grad, P.grad, 1.0, UP
    if o["api"] in ("raw", "blocks"):
        if o["api"] == "blocks":      # three blocks out of order and an empty one
            a, b = g.np_ // 3, 2 * g.np_ // 3
            extra["p_chunks"] = [(a, b, None), (0, a, None), (b, b, None), (b, g.np_, None)]
        loss, dU, dP = ops.edge_bce_loss_raw(
            t.U, t.P, t.ei, neg, None if edge else g.E,
            None if edge else torch.tensor(c, device=t.dev), neg_order=order,
            row_dtype=o["rows"], pos_weights=w if edge else None, weighting=o["weighting"], **extra)
        return loss, dU, dP, c, 1.0
    U, P = t.U.clone().requires_grad_(), t.P.clone().requires_grad_()
    loss = ops.edge_bce_loss(U, P, t.ei, neg, w, neg_order=order, row_dtype=o["rows"],
                             weighting=o["weighting"], **extra)
    (loss * UP).backward()
    return loss.detach(), U.grad, P.grad, c, UP


def _paths(g, o):
    """The case's call, and with ``logq`` the same call through the LQ kernels with a table of
    zeros, which goes first: both must meet the criterion."""
    if o["logq"]:
        yield "_lq", _run(g, o, torch.zeros(g.np_, device=DEV))
    yield "", _run(g, o)


@pytest.mark.gpu
@pytest.mark.parametrize("name,o", CASES, ids=[c[0] for c in CASES])
def test_gradients_and_loss_at_saturated_scores(name, o, monkeypatch):
    monkeypatch.setenv("HGNN_ZPACK", "1" if o["zpack"] else "0")
    g = graph(o["d"])
    for tag, (loss, dU, dP, c, up) in _paths(g, o):
        ref = reference(g, o["k"], o["weighting"], c, up)
        print(name + tag, "loss", float(loss), "float64", ref.loss)
        assert abs(float(loss) - ref.loss) <= 1e-5 * ref.loss, (float(loss), ref.loss)
        check_grads(name + tag, g, dU, dP, ref, up)


@pytest.mark.gpu
@pytest.mark.parametrize("name,o", CASES, ids=[c[0] for c in CASES])
def test_loss_of_the_all_right_side_subgraph(name, o, monkeypatch):
    monkeypatch.setenv("HGNN_ZPACK", "1" if o["zpack"] else "0")
    g = graph(o["d"], "right")
    for tag, (loss, dU, dP, c, up) in _paths(g, o):
        check_small_loss(name + tag, g, o["k"], loss, reference(g, o["k"], o["weighting"], c, up))


EXTREME_CASES = [c for c in CASES if c[0] in (
    "d64_k1", "d128_k3_edge_bf16_skewed", "d5_k1_edge", "d128_k3_edge_zpack_skewed",
    "d64_k1_logq0", "d64_k3_linkloss")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,o", EXTREME_CASES, ids=[c[0] for c in EXTREME_CASES])
def test_scores_of_100_and_10000(name, o, monkeypatch):
    monkeypatch.setenv("HGNN_ZPACK", "1" if o["zpack"] else "0")
    g = graph(o["d"], "extreme")
    for tag, (loss, dU, dP, c, up) in _paths(g, o):
        check_extreme(name + tag, g, loss, dU, dP, reference(g, o["k"], o["weighting"], c, up), up)
