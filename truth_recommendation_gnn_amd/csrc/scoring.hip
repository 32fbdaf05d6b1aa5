// Edge scoring + weighted BCE of the reference training step (train_gnn.py:259-281), fused.
//
//   s_pos[e] = <U[u_e], P[p_e]>,  s_neg[e] = <U[u_e], P[n_e]>
//   loss = mean(pos_weights) * mean_e softplus(-s_pos) + mean_e softplus(s_neg)      (default)
//   loss = mean_e(w_e * softplus(-s_pos)) + mean_e softplus(s_neg)                   (per edge)
//
// The default is the reference's own arithmetic, reproduced: BCEWithLogitsLoss() reduces to a
// scalar, so its per-edge interaction weights collapse to their mean (the device scalar c).  The
// per-edge mode (the EW instantiations, hgnn_edge_score_fwd_w) is the weighting that code meant:
// each positive edge's loss term and gradient scaled by its own weight, read per position.
//
// Pass A (this file) walks the positive edges grouped by user (the CSC of the engages relation):
// one wave per user keeps U[u] in registers, gathers P[p_e] and P[n_e] per edge, and in the same
// pass produces the loss partials AND dL/dU for a unit upstream gradient
//   dU[u] = sum_e  c/E (sigma(s_pos)-1) P[p_e] + 1/E sigma(s_neg) P[n_e]      (per edge: c w_e/E)
// with no atomics (the wave owns the row).  It also emits each edge's weights for dP:
//   hpos (written at the edge's post-grouped position) and (n_e, u_e, hneg) for the negatives.
// dP is then two K1-style weighted gathers of U rows (gather.hip): positives over the post-
// grouped CSR, negatives over the (n_e)-sorted list (hgnn_sort_pairs_i32).  Deterministic.
//
// Every kernel here and in gather.hip forms a pair's terms with bce_terms.h's helpers, from
// t = exp(-|s|):  sigma(s) - 1 as -sigma(-s) = -t/(1+t) for s >= 0 (pos_coef_t; a product, so a
// saturated positive keeps its digits where 1/(1+t) - 1 is 0 from s ~ 17), and softplus as
// max(x, 0) + log1p(t) with the rounding of 1 + t corrected (softplus_t).  Coefficients and loss
// terms are accurate relative to themselves down to the underflow of t (|s| ~ 87).
#include "hgnn_common.h"

// Post rows of the negatives (uniform draws, little reuse) are read with nt loads: cfg4 scoring
// pass 26.4 -> 25.8 ms.  The positives' rows keep the default policy: their Zipf-hot posts live on
// cache reuse (nt on both: 33.1 ms).  Measurement builds: 0 = none, 2 = both.
// Cache policy (per launch, from the table sizes): the negatives' post rows (uniform draws,
// little reuse) are read with nt loads when the post table outgrows the Infinity Cache (cfg4,
// 488 MiB: 26.4 -> 25.8 ms; the positives' Zipf-hot rows keep the default policy: nt on both
// measured 33.1 ms); the dU rows are then stored nt too.  Its own instantiation, so the
// default-policy kernel (cfg2/cfg3) is the same code as before.


namespace hgnn {

struct ScoreArgs {
  const void* U;               // fp32 rows, or bf16 rows in the XT = uint16_t instantiation
  const void* P;
  const int32_t* rowptr;       // user-grouped CSR of the positive edges
  const int32_t* col;          // post id per position
  const int64_t* neg;          // negative post id per position (user-grouped order) ...
  const int32_t* neg32;        // ... or as int32 ...
  const uint64_t* neg_seed;    // ... or drawn here: uniform_draw(*neg_seed, position, n_posts)
  const int32_t* to_post_pos;  // position -> post-grouped position (for hpos)
  const float* cscale;         // device scalar mean(pos_weights)
  float* dU;
  float* hpos;
  int32_t* neg_key;
  int32_t* neg_u;
  float* neg_w;
  float* part;                 // [gridDim.x][2]
  int32_t* err;
  int64_t n_users;
  int64_t n_posts;
  float inv_e;
  int32_t d;
  int32_t nt_neg;              // nt policy: negatives' post rows loaded, dU rows stored
  const float* edge_w;         // EW: weight of the positive edge per position (user-grouped order)
};

// XT: the element type of U and P (RowSrc).  bf16 rows are read 16 B per lane (W = 8), held packed
// in the ping-pong sets and widened to fp32 where a step is scored; dU and the loss stay fp32.
// EW: per-edge positive weights.  The lane that loads col[base + lane] loads edge_w[base + lane]
// with it (one more coalesced 256-B read per 64 edges) and the value reaches the scoring slot by
// the shuffle pid takes; hp and the edge's loss term are scaled by it, nothing else moves.
template <int LPR, int VPL, int W, bool NT = false, typename XT = float, bool EW = false>
__global__ void __launch_bounds__(256) k_edge_score(const ScoreArgs a) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  const XT* const Ux = static_cast<const XT*>(a.U);
  const XT* const Px = static_cast<const XT*>(a.P);
  constexpr int NS = 64 / LPR;
  __shared__ float red[2][4];
  // wave index through readfirstlane: u, the row bounds and n are then scalar (wave-uniform to
  // the compiler), so the step loop's exits are scalar branches and the waitcnt pass can count
  // the in-flight prefetch across them
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = lane / LPR, sl = lane % LPR;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  const float c = *a.cscale;
  const int d = a.d;
  // drawn negatives (hgnn_edge_score_fwd_draw): the draw of position k is recomputed here, so the
  // sort that groups them by post writes no position-order copy for this pass to read
  const bool seed_p = a.neg_seed != nullptr;
  const uint64_t seed = seed_p ? *a.neg_seed : 0;
  float lpos = 0.f, lneg = 0.f;   // per-lane loss sums (edge = lane)
  if (u < a.n_users) {
    const int64_t beg = a.rowptr[u], end = a.rowptr[u + 1];
    typename V::T uv[VPL], acc[VPL];
#pragma unroll
    for (int q = 0; q < VPL; ++q) {
      const int cc = (q * LPR + sl) * W;
      uv[q] = cc < d ? S::widen(S::load(Ux + u * d + cc)) : V::zero();
      acc[q] = V::zero();
    }
    for (int64_t base = beg; base < end; base += 64) {
      const int n = (int)min<int64_t>(64, end - base);
      int pid = 0, nid = 0;
      float pw = 0.f;
      if (lane < n) {
        pid = a.col[base + lane];
        if constexpr (EW) pw = a.edge_w[base + lane];
        const int64_t nn = seed_p ? (int64_t)uniform_draw(seed, base + lane, (uint32_t)a.n_posts)
                           : a.neg32 ? (int64_t)a.neg32[base + lane] : a.neg[base + lane];
        if (nn < 0 || nn >= a.n_posts) {
          if (a.err) atomicAdd(a.err, 1);
        }
        else nid = (int)nn;
      }
      float my_hp = 0.f, my_hn = 0.f;
      // Software pipeline over steps of NS edges, two register sets in ping-pong: the rows of
      // step j+NS are in flight while step j is scored, with no register copy between steps (a
      // copy reads the prefetched registers, so it made each step wait for the next one's loads).
      // Loads are unconditional: lanes past the chunk read post 0 (pid/nid are 0 there) and
      // columns past d read column 0; neither reaches a result (their hp/hn are zeroed below, uv
      // is 0 past d, and the dU store is guarded).  Under exec-mask branches the compiler's
      // waitcnt pass could not count the prefetch and waited for it before using the previous
      // step's rows.
      typename S::Raw ap[VPL], an[VPL], bp[VPL], bn[VPL];
      auto load_step = [&](int j, typename S::Raw (&xp)[VPL], typename S::Raw (&xn)[VPL]) {
        const int e = j + slot;
        const int pp = __shfl(pid, e & 63, 64), qq = __shfl(nid, e & 63, 64);
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int cc = (q * LPR + sl) * W;
          const int ccl = cc < d ? cc : 0;
          xp[q] = S::load(Px + (int64_t)pp * d + ccl);
          if constexpr (NT) xn[q] = S::load_nt(Px + (int64_t)qq * d + ccl);
          else xn[q] = S::load(Px + (int64_t)qq * d + ccl);
        }
      };
      auto score_step = [&](int j, const typename S::Raw (&rp)[VPL],
                            const typename S::Raw (&rn)[VPL]) {
        const int e = j + slot;
        typename V::T vp[VPL], vn[VPL];
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          vp[q] = S::widen(rp[q]);
          vn[q] = S::widen(rn[q]);
        }
        const float sp = slot_dot<LPR, VPL, W>(uv, vp);
        const float sn = slot_dot<LPR, VPL, W>(uv, vn);
        const float tp = exp_neg_abs(sp), tn = exp_neg_abs(sn);
        float hp = c * a.inv_e * pos_coef_t(sp, tp);
        float hn = a.inv_e * sigmoid_t(sn, tn);
        float we = 1.f;
        if constexpr (EW) {
          we = __shfl(pw, e & 63, 64);
          hp *= we;
        }
        if (e >= n) hp = hn = 0.f;
        // loss terms once per edge, on the slot's first lane: softplus(-sp) and softplus(sn), the
        // positive's weighted by an explicit fma (k_edge_score_k forms the same bits)
        if (sl == 0 && e < n) {
          if constexpr (EW) lpos = fmaf(we, softplus_t(-sp, tp), lpos);
          else lpos += softplus_t(-sp, tp);
          lneg += softplus_t(sn, tn);
        }
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          V::fma(acc[q], hp, vp[q]);
          V::fma(acc[q], hn, vn[q]);
        }
        // hand edge e's weights to lane e (lanes j .. j+NS-1 read from slot lane*LPR)
        const int src = ((lane - j) & (NS - 1)) * LPR;
        const float thp = __shfl(hp, src, 64), thn = __shfl(hn, src, 64);
        if (lane >= j && lane < j + NS) {
          my_hp = thp; my_hn = thn;
        }
      };
      load_step(0, ap, an);
      for (int j = 0; j < n; j += 2 * NS) {
        load_step(j + NS, bp, bn);
        score_step(j, ap, an);
        if (j + NS >= n) break;
        load_step(j + 2 * NS, ap, an);
        score_step(j + NS, bp, bn);
      }
      if (lane < n) {
        const int64_t k = base + lane;
        if (a.hpos) a.hpos[a.to_post_pos[k]] = my_hp;
        if (a.neg_key) {
          a.neg_key[k] = nid;
          a.neg_u[k] = (int32_t)u;
        }
        if (a.neg_w) a.neg_w[k] = my_hn;
      }
    }
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1)
#pragma unroll
      for (int q = 0; q < VPL; ++q) V::add(acc[q], V::shfl_xor(acc[q], m));
    if (lane < LPR) {
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        const int cc = (q * LPR + sl) * W;
        if (cc < d) {
          if constexpr (NT) V::store_nt(a.dU + u * d + cc, acc[q]);
          else V::store(a.dU + u * d + cc, acc[q]);
        }
      }
    }
  }
  // deterministic block partials: wave tree, then waves in order
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lpos += __shfl_xor(lpos, m, 64);
    lneg += __shfl_xor(lneg, m, 64);
  }
  if (lane == 0) {
    red[0][wave] = lpos;
    red[1][wave] = lneg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[2 * blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    a.part[2 * blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// k negatives per positive edge (hgnn_edge_score_fwd_k): the arguments of k_edge_score and n_neg.
// Its own struct and its own kernel, so the one-negative instantiations above are the same code
// as before.  The negatives are row-major [E, n_neg] in the user-grouped order: negative j of
// position p is element p * n_neg + j (drawn: uniform_draw(seed, p * n_neg + j, n_posts)).  The
// caller folds the two means into the existing scales: inv_e = 1 / (E * n_neg) and
// *cscale = c * n_neg, so a positive edge weighs c / E and a negative 1 / (E * n_neg).
struct ScoreArgsK {
  ScoreArgs s;
  int32_t n_neg;
  const float* post_bias;      // LQ: the per-post offset of the logits (fp32 [n_posts]), else null
};

// One wave per user, U[u] in registers, as k_edge_score.  A 64-edge chunk is walked in sweeps of
// the same two-set ping-pong: the first sweep is k_edge_score's two-row step (the positive row and
// negative 0 of NS edges per step: with n_neg = 1 the same operations in the same order), then
// every further pair of negative columns takes one sweep of two rows per edge, and an odd last
// column a sweep of one.  So P[p_e] is read once and each P[n_e,j] once, all into the one dU
// accumulator the wave owns.  A sweep's ids (lane = edge: neg[(base + lane) * n_neg + j], the
// 64 * n_neg ids of a chunk being contiguous) are loaded before the previous sweep runs.  An
// out-of-range id is counted into err and kept as -1: its row load reads post 0 and its weight
// and loss term are zeroed.  hpos / neg_key / neg_w are not written.
//
// LQ (hgnn_edge_score_fwd_k_lq): every scored pair's logit is <U[u], P[p]> - post_bias[p].  The
// lane that holds an edge's id for a sweep loads post_bias[id] where the id becomes available (the
// positive's with col, a negative's where its sweep checks the id: the 4-byte dependent read is
// issued ahead of the sweep's first rows and is older than they are, so the first step's wait for
// its rows covers it); an id kept as -1 reads entry 0, as its row load reads post 0.  The value
// reaches the scoring slot by the shuffle the id takes and is subtracted from the dot product
// before exp_neg_abs; the rows, the sums into dU and their order are unchanged, and so are the
// expressions of the coefficients and the loss terms (bce_terms.h, one spelling for every path:
// a table of zeros gives the numbers of the call without one).  Its own instantiations.
template <int LPR, int VPL, int W, bool NT = false, typename XT = float, bool EW = false,
          bool LQ = false>
__global__ void __launch_bounds__(256) k_edge_score_k(const ScoreArgsK ak) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  using Raw = typename S::Raw;
  using Yes = std::true_type;
  using No = std::false_type;
  const ScoreArgs& a = ak.s;
  const int K = ak.n_neg;
  const XT* const Ux = static_cast<const XT*>(a.U);
  const XT* const Px = static_cast<const XT*>(a.P);
  constexpr int NS = 64 / LPR;
  __shared__ float red[2][4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = lane / LPR, sl = lane % LPR;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  const float c = *a.cscale;
  const int d = a.d;
  const bool seed_p = a.neg_seed != nullptr;
  const uint64_t seed = seed_p ? *a.neg_seed : 0;
  float lpos = 0.f, lneg = 0.f;   // per-lane loss sums, on each slot's first lane
  if (u < a.n_users) {
    const int64_t beg = a.rowptr[u], end = a.rowptr[u + 1];
    typename V::T uv[VPL], acc[VPL];
#pragma unroll
    for (int q = 0; q < VPL; ++q) {
      const int cc = (q * LPR + sl) * W;
      uv[q] = cc < d ? S::widen(S::load(Ux + u * d + cc)) : V::zero();
      acc[q] = V::zero();
    }
    for (int64_t base = beg; base < end; base += 64) {
      const int n = (int)min<int64_t>(64, end - base);
      int pid = 0;
      float pw = 0.f;
      if (lane < n) {
        pid = a.col[base + lane];
        if constexpr (EW) pw = a.edge_w[base + lane];
      }
      // the offset of an id this lane holds (unconditional, as the row loads are: -1 reads entry 0)
      auto bias_of = [&](int id) -> float {
        if constexpr (LQ) return ak.post_bias[max(id, 0)];
        else return 0.f;
      };
      const float pq = bias_of(pid);
      // column j of this lane's edge as loaded (or drawn), checked only where its sweep starts:
      // the check waits for the load, the load is issued a sweep ahead
      auto raw_neg = [&](int j) -> int64_t {
        if (lane >= n) return 0;
        const int64_t i = (base + lane) * K + j;
        return seed_p ? (int64_t)uniform_draw(seed, i, (uint32_t)a.n_posts)
               : a.neg32 ? (int64_t)a.neg32[i] : a.neg[i];
      };
      auto checked = [&](int64_t nn) -> int {
        if (nn < 0 || nn >= a.n_posts) {
          if (a.err) atomicAdd(a.err, 1);
          return -1;
        }
        return (int)nn;
      };
      // The steps of k_edge_score (its comment on the unconditional loads holds here), over the
      // rows of one sweep: row 0 is the positive (pos0) or a negative, row 1 (two) a negative.
      Raw a0[VPL], a1[VPL], b0[VPL], b1[VPL];
      auto load_step = [&](auto pos0, auto two, int j, int id0, int id1, Raw (&x0)[VPL],
                           Raw (&x1)[VPL]) {
        const int e = j + slot;
        const int r0 = max(__shfl(id0, e & 63, 64), 0);
        int r1 = 0;
        if constexpr (two) r1 = max(__shfl(id1, e & 63, 64), 0);
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int cc = (q * LPR + sl) * W;
          const int ccl = cc < d ? cc : 0;
          if constexpr (NT && !pos0) x0[q] = S::load_nt(Px + (int64_t)r0 * d + ccl);
          else x0[q] = S::load(Px + (int64_t)r0 * d + ccl);
          if constexpr (two) {
            if constexpr (NT) x1[q] = S::load_nt(Px + (int64_t)r1 * d + ccl);
            else x1[q] = S::load(Px + (int64_t)r1 * d + ccl);
          }
        }
      };
      auto score_step = [&](auto pos0, auto two, int j, int id0, int id1, float q0, float q1,
                            const Raw (&r0)[VPL], const Raw (&r1)[VPL]) {
        const int e = j + slot;
        typename V::T v0[VPL], v1[VPL];
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          v0[q] = S::widen(r0[q]);
          if constexpr (two) v1[q] = S::widen(r1[q]);
        }
        float s0 = slot_dot<LPR, VPL, W>(uv, v0);
        float s1 = 0.f;
        if constexpr (two) s1 = slot_dot<LPR, VPL, W>(uv, v1);
        if constexpr (LQ) {   // the logit: the score less the row's post's offset
          s0 -= __shfl(q0, e & 63, 64);
          if constexpr (two) s1 -= __shfl(q1, e & 63, 64);
        }
        const float t0 = exp_neg_abs(s0), t1 = exp_neg_abs(s1);
        float h0, h1 = 0.f;
        bool ok0 = e < n, ok1 = e < n;
        if constexpr (pos0) {
          // sigmoid(z) - 1 as -sigmoid(-z) (pos_coef_t): a trained model's positives, or an offset
          // of log(1/T) (a post of weight 0, PostDistribution.log_q), sit at z of 17 and more,
          // where 1/(1 + t) - 1 is exactly 0 in fp32 and the edge would push nothing
          h0 = c * a.inv_e * pos_coef_t(s0, t0);
        } else {
          h0 = a.inv_e * sigmoid_t(s0, t0);
          ok0 = ok0 && __shfl(id0, e & 63, 64) >= 0;
        }
        if constexpr (two) {
          h1 = a.inv_e * sigmoid_t(s1, t1);
          ok1 = ok1 && __shfl(id1, e & 63, 64) >= 0;
        }
        float we = 1.f;
        if constexpr (EW && pos0) {
          we = __shfl(pw, e & 63, 64);
          h0 *= we;
        }
        if (!ok0) h0 = 0.f;
        if (!ok1) h1 = 0.f;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          V::fma(acc[q], h0, v0[q]);
          if constexpr (two) V::fma(acc[q], h1, v1[q]);
        }
        // loss terms once per row, on the slot's first lane (k_edge_score's expressions), after
        // the rows' last use: the terms' temporaries then take the registers the rows leave
        if (sl == 0) {
          if constexpr (pos0) {
            if (ok0) {
              // (the explicit fma of k_edge_score: the same bits whatever the compiler contracts)
              if constexpr (EW) lpos = fmaf(we, softplus_t(-s0, t0), lpos);
              else lpos += softplus_t(-s0, t0);
            }
          } else {
            if (ok0) lneg += softplus_t(s0, t0);
          }
          if constexpr (two) {
            if (ok1) lneg += softplus_t(s1, t1);
          }
        }
      };
      auto sweep = [&](auto pos0, auto two, int id0, int id1, float q0, float q1) {
        load_step(pos0, two, 0, id0, id1, a0, a1);
        for (int j = 0; j < n; j += 2 * NS) {
          load_step(pos0, two, j + NS, id0, id1, b0, b1);
          score_step(pos0, two, j, id0, id1, q0, q1, a0, a1);
          if (j + NS >= n) break;
          load_step(pos0, two, j + 2 * NS, id0, id1, a0, a1);
          score_step(pos0, two, j + NS, id0, id1, q0, q1, b0, b1);
        }
      };
      const int nid = checked(raw_neg(0));
      const float nq = bias_of(nid);
      int j = 1;
      int64_t rw0 = 0, rw1 = 0;
      if (j < K) rw0 = raw_neg(j);
      if (j + 1 < K) rw1 = raw_neg(j + 1);
      sweep(Yes{}, Yes{}, pid, nid, pq, nq);
      while (j + 1 < K) {
        const int i0 = checked(rw0), i1 = checked(rw1);
        const float q0 = bias_of(i0), q1 = bias_of(i1);
        j += 2;
        if (j < K) rw0 = raw_neg(j);
        if (j + 1 < K) rw1 = raw_neg(j + 1);
        sweep(No{}, Yes{}, i0, i1, q0, q1);
      }
      if (j < K) {
        const int i0 = checked(rw0);
        sweep(No{}, No{}, i0, 0, bias_of(i0), 0.f);
      }
    }
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1)
#pragma unroll
      for (int q = 0; q < VPL; ++q) V::add(acc[q], V::shfl_xor(acc[q], m));
    if (lane < LPR) {
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        const int cc = (q * LPR + sl) * W;
        if (cc < d) {
          if constexpr (NT) V::store_nt(a.dU + u * d + cc, acc[q]);
          else V::store(a.dU + u * d + cc, acc[q]);
        }
      }
    }
  }
  // deterministic block partials, as k_edge_score: wave tree, then waves in order
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lpos += __shfl_xor(lpos, m, 64);
    lneg += __shfl_xor(lneg, m, 64);
  }
  if (lane == 0) {
    red[0][wave] = lpos;
    red[1][wave] = lneg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[2 * blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    a.part[2 * blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// Deterministic two-level reduction of the block partials: 64 blocks each sum a contiguous
// range (double), then one block sums the 64 and forms the loss.
constexpr int kRedBlocks = 64;

__global__ void __launch_bounds__(256) k_loss_partial(const float* part, int64_t n_part,
                                                      double* red) {
  __shared__ double sp[256], sn[256];
  const int64_t per = cdiv(n_part, kRedBlocks);
  const int64_t b0 = blockIdx.x * per, b1 = min<int64_t>(b0 + per, n_part);
  double p = 0.0, q = 0.0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) {
    p += part[2 * i];
    q += part[2 * i + 1];
  }
  sp[threadIdx.x] = p;
  sn[threadIdx.x] = q;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sp[threadIdx.x] += sp[threadIdx.x + s];
      sn[threadIdx.x] += sn[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    red[2 * blockIdx.x] = sp[0];
    red[2 * blockIdx.x + 1] = sn[0];
  }
}

// loss = c * inv_e * sum(pos) + inv_e * sum(neg)
__global__ void k_loss_final(const double* red, const float* cscale, float inv_e, float* loss) {
  if (threadIdx.x != 0) return;
  double p = 0.0, q = 0.0;
  for (int i = 0; i < kRedBlocks; ++i) {
    p += red[2 * i];
    q += red[2 * i + 1];
  }
  *loss = (float)((double)*cscale * (double)inv_e * p + (double)inv_e * q);
}

// k_loss_partial + k_loss_final in one block (few partials: a sampled batch's loss), bitwise the
// same sums: wave w takes virtual blocks 4w .. 4w + 3; lane l stands for the partial kernel's
// threads l, l + 64, l + 128, l + 192 (the same strided double sums), the shared-memory tree's
// first two levels are in-lane adds and the other six shuffles in the same order; the 64 block
// sums are then added in order as k_loss_final does.
__global__ void __launch_bounds__(1024) k_loss_one(const float* part, int64_t n_part,
                                                   const float* cscale, float inv_e,
                                                   float* loss) {
  __shared__ double red[2 * kRedBlocks];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t per = cdiv(n_part, kRedBlocks);
  for (int vb = 4 * wv; vb < 4 * wv + 4; ++vb) {
    const int64_t b0 = vb * per, b1 = min<int64_t>(b0 + per, n_part);
    double p[4], q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p[k] = 0.0;
      q[k] = 0.0;
      for (int64_t i = b0 + lane + 64 * k; i < b1; i += 256) {
        p[k] += part[2 * i];
        q[k] += part[2 * i + 1];
      }
    }
    // s = 128: t += t + 128 (slots 0, 1 take 2, 3); s = 64: slot 0 takes slot 1
    p[0] += p[2]; q[0] += q[2];
    p[1] += p[3]; q[1] += q[3];
    p[0] += p[1]; q[0] += q[1];
    double pp = p[0], qq = q[0];
    for (int s = 32; s > 0; s >>= 1) {   // t += t + s for t < s (lanes >= s carry don't-cares)
      const double po = __shfl_down(pp, s, 64), qo = __shfl_down(qq, s, 64);
      if (lane < s) {
        pp += po;
        qq += qo;
      }
    }
    if (lane == 0) {
      red[2 * vb] = pp;
      red[2 * vb + 1] = qq;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ps = 0.0, qs = 0.0;
    for (int i = 0; i < kRedBlocks; ++i) {
      ps += red[2 * i];
      qs += red[2 * i + 1];
    }
    *loss = (float)((double)*cscale * (double)inv_e * ps + (double)inv_e * qs);
  }
}

// few enough partials for one block to sum them faster than two launches
constexpr int64_t kLossOneMax = 65536;
// the rule by users (one partial per block of 4 user-waves): hgnn_loss_one_pass
static bool loss_one_pass(int64_t n_users) { return cdiv(n_users, 4) <= kLossOneMax; }

// The nt policy of the scoring pass (ScoreArgs::nt_neg, hgnn_score_nt_policy): on where the post
// table, in the bytes of its stored dtype, outgrows the Infinity Cache.
constexpr int64_t kScoreNtBytes = int64_t(256) << 20;
static bool score_nt_policy(int64_t n_posts, int32_t d, bool bf16) {
  return n_posts * d * (bf16 ? 2 : 4) >= kScoreNtBytes;
}

template <int LPR, int VPL, int W, typename XT, bool NT, bool EW, bool LQ = false>
static int launch_score_k(const ScoreArgs& a, int32_t n_neg, int64_t nblocks, hipStream_t stream,
                          const float* post_bias = nullptr) {
  const ScoreArgsK ak{a, n_neg, post_bias};
  hipLaunchKernelGGL((k_edge_score_k<LPR, VPL, W, NT, XT, EW, LQ>), dim3((unsigned)nblocks),
                     dim3(256), 0, stream, ak);
  return check_launch(LQ ? "k_edge_score_k(lq)" : "k_edge_score_k");
}

// n_neg > 0: the k-negative kernel (hgnn_edge_score_fwd_k), under the same two choices;
// post_bias (with n_neg > 0 only): its LQ instantiations (hgnn_edge_score_fwd_k_lq)
template <int LPR, int VPL, int W, typename XT = float>
static int launch_score(const ScoreArgs& a, int64_t nblocks, hipStream_t stream,
                        int32_t n_neg = 0, const float* post_bias = nullptr) {
  if (n_neg > 0 && post_bias) {
    const float* b = post_bias;
    if (a.edge_w)
      return a.nt_neg
                 ? launch_score_k<LPR, VPL, W, XT, true, true, true>(a, n_neg, nblocks, stream, b)
                 : launch_score_k<LPR, VPL, W, XT, false, true, true>(a, n_neg, nblocks, stream, b);
    return a.nt_neg
               ? launch_score_k<LPR, VPL, W, XT, true, false, true>(a, n_neg, nblocks, stream, b)
               : launch_score_k<LPR, VPL, W, XT, false, false, true>(a, n_neg, nblocks, stream, b);
  }
  if (n_neg > 0) {
    if (a.edge_w)
      return a.nt_neg ? launch_score_k<LPR, VPL, W, XT, true, true>(a, n_neg, nblocks, stream)
                      : launch_score_k<LPR, VPL, W, XT, false, true>(a, n_neg, nblocks, stream);
    return a.nt_neg ? launch_score_k<LPR, VPL, W, XT, true, false>(a, n_neg, nblocks, stream)
                    : launch_score_k<LPR, VPL, W, XT, false, false>(a, n_neg, nblocks, stream);
  }
  if (a.edge_w) {   // per-edge weights: their own instantiations too, under either policy
    if (a.nt_neg)
      hipLaunchKernelGGL((k_edge_score<LPR, VPL, W, true, XT, true>), dim3((unsigned)nblocks),
                         dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((k_edge_score<LPR, VPL, W, false, XT, true>), dim3((unsigned)nblocks),
                         dim3(256), 0, stream, a);
    return check_launch("k_edge_score");
  }
  if (a.nt_neg)   // the cache policy as its own instantiation: the default one is unchanged
    hipLaunchKernelGGL((k_edge_score<LPR, VPL, W, true, XT>), dim3((unsigned)nblocks), dim3(256),
                       0, stream, a);
  else
    hipLaunchKernelGGL((k_edge_score<LPR, VPL, W, false, XT>), dim3((unsigned)nblocks),
                       dim3(256), 0, stream, a);
  return check_launch("k_edge_score");
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

// floats of `part` scratch: 2 per block (4 users) + room for 2*64 doubles, 16-B aligned
int64_t hgnn_edge_score_parts(int64_t n_users) {
  return (int64_t)align_up((size_t)(2 * cdiv(n_users, 4)), 4) + 4 * kRedBlocks;
}

int32_t hgnn_score_nt_policy(int64_t n_posts, int32_t d, int32_t bf16) {
  return score_nt_policy(n_posts, d, bf16 != 0) ? 1 : 0;
}

int32_t hgnn_loss_one_pass(int64_t n_users) { return loss_one_pass(n_users) ? 1 : 0; }

// `bf16`: U and P hold bf16 rows (hgnn_edge_score_fwd_bf16); `edge_w`: the per-edge weights of
// the _w entries (null: the collapsed weighting, c alone); `n_neg` > 0: the _k entries' kernel;
// `post_bias`: the _k_lq entries' offsets (with n_neg > 0)
static int edge_score_fwd(const void* U, const void* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const int64_t* neg_u_order, const int32_t* neg32,
                          const uint64_t* neg_seed, const int32_t* to_post_pos, int64_t n_edges, const float* cscale,
                          float* dU, float* hpos, int32_t* neg_key, int32_t* neg_user,
                          float* neg_w, float* part, float* loss, int32_t* err,
                          hgnn_stream_t stream_, bool bf16 = false,
                          const float* edge_w = nullptr, int32_t n_neg = 0,
                          const float* post_bias = nullptr) {
  hipStream_t stream = as_stream(stream_);
  if (d < 1 || n_users < 0 || n_posts < 0 || n_edges < 0)
    return fail(HGNN_E_ARG, "edge_score: bad sizes");
  if (!cscale || !loss ||
      (n_users > 0 && (!U || !rowptr_u || !dU || !part)) || (!neg_key != !neg_user))
    return fail(HGNN_E_ARG, "edge_score: null pointer");
  if (hpos && !to_post_pos) return fail(HGNN_E_ARG, "edge_score: hpos needs to_post_pos");
  if (err) (void)hipMemsetAsync(err, 0, sizeof(int32_t), stream);   // (null: not counted)
  ScoreArgs a{};
  a.U = U; a.P = P; a.rowptr = rowptr_u; a.col = col_u; a.neg = neg_u_order; a.neg32 = neg32;
  a.neg_seed = neg_seed; a.edge_w = edge_w;
  a.to_post_pos = to_post_pos; a.cscale = cscale; a.dU = dU; a.hpos = hpos; a.neg_key = neg_key;
  a.neg_u = neg_user; a.neg_w = neg_w; a.part = part; a.err = err; a.n_users = n_users;
  a.n_posts = n_posts; a.inv_e = n_edges > 0 ? 1.f / (float)n_edges : 0.f; a.d = d;
  a.nt_neg = score_nt_policy(n_posts, d, bf16) ? 1 : 0;
  const int64_t nb = cdiv(n_users, 4);   // blocks of 4 user-waves
  int rc = HGNN_OK;
  if (nb > 0) {
    // one 4..16-edge step per iteration, next step's loads pipelined (an unrolled 2-step body
    // measured slower: users average ~20 edges, so wider steps waste the tail)
    if (bf16) {   // 16 B = 8 elements per lane: d = 128 is 16 lanes per row, 4 edges per step
      using B = uint16_t;
      if (d <= 64) rc = launch_score<8, 1, 8, B>(a, nb, stream, n_neg, post_bias);
      else if (d <= 128) rc = launch_score<16, 1, 8, B>(a, nb, stream, n_neg, post_bias);
      else if (d <= 256) rc = launch_score<32, 1, 8, B>(a, nb, stream, n_neg, post_bias);
      else rc = launch_score<64, 1, 8, B>(a, nb, stream, n_neg, post_bias);
    }
    else if (d % 4 == 0 && d <= 64) rc = launch_score<16, 1, 4>(a, nb, stream, n_neg, post_bias);
    else if (d % 4 == 0 && d <= 128) rc = launch_score<32, 1, 4>(a, nb, stream, n_neg, post_bias);
    else if (d % 4 == 0 && d <= 256) rc = launch_score<64, 1, 4>(a, nb, stream, n_neg, post_bias);
    else if (d <= 64) rc = launch_score<64, 1, 1>(a, nb, stream, n_neg, post_bias);
    else if (d <= 512) rc = launch_score<64, 8, 1>(a, nb, stream, n_neg, post_bias);
    else return fail(HGNN_E_UNSUPPORTED, "edge_score: d=%d", d);
    if (rc) return rc;
  }
  // the reduction scratch lives after the block partials: part holds 2*nb floats + 2*64 doubles
  double* red = reinterpret_cast<double*>(part + align_up((size_t)(2 * nb), 4));
  if (loss_one_pass(n_users)) {
    hipLaunchKernelGGL(k_loss_one, dim3(1), dim3(1024), 0, stream, part, nb, cscale, a.inv_e,
                       loss);
    return check_launch("k_loss_one");
  }
  hipLaunchKernelGGL(k_loss_partial, dim3(kRedBlocks), dim3(256), 0, stream, part, nb, red);
  if (int rc2 = check_launch("k_loss_partial")) return rc2;
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(64), 0, stream, red, cscale, a.inv_e, loss);
  return check_launch("k_loss_final");
}

int hgnn_edge_score_fwd(const float* U, const float* P, int32_t d, int64_t n_users,
                        int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                        const int64_t* neg_u_order, const int32_t* to_post_pos, int64_t n_edges,
                        const float* cscale, float* dU, float* hpos, int32_t* neg_key,
                        int32_t* neg_user, float* neg_w, float* part, float* loss, int32_t* err,
                        hgnn_stream_t stream) {
  if (n_edges > 0 && !neg_u_order) return fail(HGNN_E_ARG, "edge_score: negatives are null");
  return edge_score_fwd(U, P, d, n_users, n_posts, rowptr_u, col_u, neg_u_order, nullptr,
                        nullptr, to_post_pos, n_edges, cscale, dU, hpos, neg_key, neg_user, neg_w, part,
                        loss, err, stream);
}

int hgnn_edge_score_fwd_i32(const float* U, const float* P, int32_t d, int64_t n_users,
                            int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                            const int32_t* neg_u_order, int64_t n_edges, const float* cscale,
                            float* dU, float* part, float* loss, int32_t* err,
                            hgnn_stream_t stream) {
  if (n_edges > 0 && !neg_u_order) return fail(HGNN_E_ARG, "edge_score: negatives are null");
  return edge_score_fwd(U, P, d, n_users, n_posts, rowptr_u, col_u, nullptr, neg_u_order,
                        nullptr, nullptr, n_edges, cscale, dU, nullptr, nullptr, nullptr, nullptr, part,
                        loss, err, stream);
}

int hgnn_edge_score_fwd_draw(const float* U, const float* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const uint64_t* d_seed, int64_t n_edges, const float* cscale,
                             float* dU, float* part, float* loss, int32_t* err,
                             hgnn_stream_t stream) {
  if (n_edges > 0 && !d_seed) return fail(HGNN_E_ARG, "edge_score: the draw's seed is null");
  if (n_posts < 1 || n_posts >= (int64_t(1) << 31) - 1)
    return fail(HGNN_E_ARG, "edge_score_draw: n_posts=%lld out of range", (long long)n_posts);
  return edge_score_fwd(U, P, d, n_users, n_posts, rowptr_u, col_u, nullptr, nullptr, d_seed,
                        nullptr, n_edges, cscale, dU, nullptr, nullptr, nullptr, nullptr, part,
                        loss, err, stream);
}

int hgnn_edge_score_fwd_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const int64_t* neg_i64, const int32_t* neg_i32,
                             const uint64_t* d_seed, int64_t n_edges, const float* cscale,
                             float* dU, float* part, float* loss, int32_t* err,
                             hgnn_stream_t stream) {
  if (d > 0 && (d % 8 != 0 || d > 512))
    return fail(HGNN_E_UNSUPPORTED,
                "edge_score_fwd_bf16: d=%d (bf16 rows need d %% 8 == 0 and d <= 512)", d);
  const int given = (neg_i64 != nullptr) + (neg_i32 != nullptr) + (d_seed != nullptr);
  if (given > 1 || (n_edges > 0 && given != 1))
    return fail(HGNN_E_ARG, "edge_score_fwd_bf16: the negatives come in exactly one form "
                            "(int64, int32 or a seed)");
  if (d_seed && (n_posts < 1 || n_posts >= (int64_t(1) << 31) - 1))
    return fail(HGNN_E_ARG, "edge_score_fwd_bf16: n_posts=%lld out of range for drawn negatives",
                (long long)n_posts);
  return edge_score_fwd(U, P, d, n_users, n_posts, rowptr_u, col_u, neg_i64, neg_i32, d_seed,
                        nullptr, n_edges, cscale, dU, nullptr, nullptr, nullptr, nullptr, part,
                        loss, err, stream, true);
}

// The per-edge entries: the argument rules of hgnn_edge_score_fwd_bf16 (`who` words them), then
// the weights' own, all before any launch.
static int edge_score_fwd_w(const char* who, bool bf16, const void* U, const void* P, int32_t d,
                            int64_t n_users, int64_t n_posts, const int32_t* rowptr_u,
                            const int32_t* col_u, const float* edge_w, const int64_t* neg_i64,
                            const int32_t* neg_i32, const uint64_t* d_seed, int64_t n_edges,
                            const float* cscale, float* dU, float* part, float* loss,
                            int32_t* err, hgnn_stream_t stream) {
  if (bf16 && d > 0 && (d % 8 != 0 || d > 512))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (bf16 rows need d %% 8 == 0 and d <= 512)", who, d);
  if (!bf16 && d > 512) return fail(HGNN_E_UNSUPPORTED, "edge_score: d=%d", d);
  const int given = (neg_i64 != nullptr) + (neg_i32 != nullptr) + (d_seed != nullptr);
  if (given > 1 || (n_edges > 0 && given != 1))
    return fail(HGNN_E_ARG, "%s: the negatives come in exactly one form (int64, int32 or a seed)",
                who);
  if (d_seed && (n_posts < 1 || n_posts >= (int64_t(1) << 31) - 1))
    return fail(HGNN_E_ARG, "%s: n_posts=%lld out of range for drawn negatives", who,
                (long long)n_posts);
  if (!edge_w && n_users > 0 && n_edges > 0) return fail(HGNN_E_ARG, "%s: edge_w is null", who);
  return edge_score_fwd(U, P, d, n_users, n_posts, rowptr_u, col_u, neg_i64, neg_i32, d_seed,
                        nullptr, n_edges, cscale, dU, nullptr, nullptr, nullptr, nullptr, part,
                        loss, err, stream, bf16, edge_w);
}

int hgnn_edge_score_fwd_w(const float* U, const float* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                          const uint64_t* d_seed, int64_t n_edges, const float* cscale, float* dU,
                          float* part, float* loss, int32_t* err, hgnn_stream_t stream) {
  return edge_score_fwd_w("edge_score_fwd_w", false, U, P, d, n_users, n_posts, rowptr_u, col_u,
                          edge_w, neg_i64, neg_i32, d_seed, n_edges, cscale, dU, part, loss, err,
                          stream);
}

int hgnn_edge_score_fwd_w_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                               int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                               const float* edge_w, const int64_t* neg_i64,
                               const int32_t* neg_i32, const uint64_t* d_seed, int64_t n_edges,
                               const float* cscale, float* dU, float* part, float* loss,
                               int32_t* err, hgnn_stream_t stream) {
  return edge_score_fwd_w("edge_score_fwd_w_bf16", true, U, P, d, n_users, n_posts, rowptr_u,
                          col_u, edge_w, neg_i64, neg_i32, d_seed, n_edges, cscale, dU, part,
                          loss, err, stream);
}

// The k-negative entries: the argument rules of the _w entries under the entry's own name, with
// edge_w optional, then n_neg's; all before any launch.
static int edge_score_fwd_k(const char* who, bool bf16, const void* U, const void* P, int32_t d,
                            int64_t n_users, int64_t n_posts, const int32_t* rowptr_u,
                            const int32_t* col_u, const float* edge_w, const int64_t* neg_i64,
                            const int32_t* neg_i32, const uint64_t* d_seed, int32_t n_neg,
                            int64_t n_edges, const float* cscale, float* dU, float* part,
                            float* loss, int32_t* err, hgnn_stream_t stream,
                            const float* post_bias = nullptr) {
  if (n_neg < 1) return fail(HGNN_E_ARG, "%s: n_neg=%d (at least one negative per edge)", who,
                             n_neg);
  if (bf16 && d > 0 && (d % 8 != 0 || d > 512))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (bf16 rows need d %% 8 == 0 and d <= 512)", who, d);
  if (!bf16 && d > 512)
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (fp32 rows need d <= 512)", who, d);
  const int given = (neg_i64 != nullptr) + (neg_i32 != nullptr) + (d_seed != nullptr);
  if (given > 1 || (n_edges > 0 && given != 1))
    return fail(HGNN_E_ARG, "%s: the negatives come in exactly one form (int64, int32 or a seed)",
                who);
  if (d_seed && (n_posts < 1 || n_posts >= (int64_t(1) << 31) - 1))
    return fail(HGNN_E_ARG, "%s: n_posts=%lld out of range for drawn negatives", who,
                (long long)n_posts);
  return edge_score_fwd(U, P, d, n_users, n_posts, rowptr_u, col_u, neg_i64, neg_i32, d_seed,
                        nullptr, n_edges, cscale, dU, nullptr, nullptr, nullptr, nullptr, part,
                        loss, err, stream, bf16, edge_w, n_neg, post_bias);
}

int hgnn_edge_score_fwd_k(const float* U, const float* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                          const uint64_t* d_seed, int32_t n_neg, int64_t n_edges,
                          const float* cscale, float* dU, float* part, float* loss, int32_t* err,
                          hgnn_stream_t stream) {
  return edge_score_fwd_k("edge_score_fwd_k", false, U, P, d, n_users, n_posts, rowptr_u, col_u,
                          edge_w, neg_i64, neg_i32, d_seed, n_neg, n_edges, cscale, dU, part,
                          loss, err, stream);
}

int hgnn_edge_score_fwd_k_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                               int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                               const float* edge_w, const int64_t* neg_i64,
                               const int32_t* neg_i32, const uint64_t* d_seed, int32_t n_neg,
                               int64_t n_edges, const float* cscale, float* dU, float* part,
                               float* loss, int32_t* err, hgnn_stream_t stream) {
  return edge_score_fwd_k("edge_score_fwd_k_bf16", true, U, P, d, n_users, n_posts, rowptr_u,
                          col_u, edge_w, neg_i64, neg_i32, d_seed, n_neg, n_edges, cscale, dU,
                          part, loss, err, stream);
}

// The logQ entries: post_bias's own rule, then those of the _k entries under this entry's name.
int hgnn_edge_score_fwd_k_lq(const float* U, const float* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                             const uint64_t* d_seed, int32_t n_neg, int64_t n_edges,
                             const float* cscale, const float* post_bias, float* dU, float* part,
                             float* loss, int32_t* err, hgnn_stream_t stream) {
  if (!post_bias) return fail(HGNN_E_ARG, "edge_score_fwd_k_lq: post_bias is null");
  return edge_score_fwd_k("edge_score_fwd_k_lq", false, U, P, d, n_users, n_posts, rowptr_u,
                          col_u, edge_w, neg_i64, neg_i32, d_seed, n_neg, n_edges, cscale, dU,
                          part, loss, err, stream, post_bias);
}

int hgnn_edge_score_fwd_k_lq_bf16(const uint16_t* U, const uint16_t* P, int32_t d,
                                  int64_t n_users, int64_t n_posts, const int32_t* rowptr_u,
                                  const int32_t* col_u, const float* edge_w,
                                  const int64_t* neg_i64, const int32_t* neg_i32,
                                  const uint64_t* d_seed, int32_t n_neg, int64_t n_edges,
                                  const float* cscale, const float* post_bias, float* dU,
                                  float* part, float* loss, int32_t* err, hgnn_stream_t stream) {
  if (!post_bias) return fail(HGNN_E_ARG, "edge_score_fwd_k_lq_bf16: post_bias is null");
  return edge_score_fwd_k("edge_score_fwd_k_lq_bf16", true, U, P, d, n_users, n_posts, rowptr_u,
                          col_u, edge_w, neg_i64, neg_i32, d_seed, n_neg, n_edges, cscale, dU,
                          part, loss, err, stream, post_bias);
}

// Uniform draws in [0, hi): out[i] = hi * (splitmix64(seed + i * golden) >> 32) >> 32 (Lemire's
// multiply-shift), the seed read from device memory so the caller draws it from a torch
// Generator without a host sync.  The loss's negatives (train_gnn.py:272's torch.randint) drawn
// as int32 in range by construction: no int64 array, no validation pass before the sort.
__global__ void k_uniform_i32(const uint64_t* seed, int64_t n, uint32_t hi, int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = uniform_draw(*seed, i, hi);
}

// x *= *s in place, skipped entirely when *s == 1 (read on the device: no host sync).  The
// loss's backward scales its precomputed dU/dP by the incoming gradient, which is exactly 1 for
// loss.backward(); the early exit turns a 256 MB read-modify-write into one launch.
__global__ void k_scale_unless_one(float* x, int64_t n, const float* s) {
  const float g = *s;
  if (g == 1.0f) return;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float4* x4 = reinterpret_cast<float4*>(x);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = x4[i];
    v.x *= g; v.y *= g; v.z *= g; v.w *= g;
    x4[i] = v;
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    x[i] *= g;
}

int hgnn_scale_unless_one(float* x, int64_t n, const float* d_scale, hgnn_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  if (n < 0) return fail(HGNN_E_ARG, "scale_unless_one: n=%lld", (long long)n);
  if (n == 0) return HGNN_OK;
  if (!x || !d_scale) return fail(HGNN_E_ARG, "scale_unless_one: null pointer");
  if (reinterpret_cast<uintptr_t>(x) & 15)
    return fail(HGNN_E_ARG, "scale_unless_one: x must be 16-byte aligned");
  const int64_t blocks = std::min<int64_t>(cdiv(cdiv(n, 4), 256), 2048);
  hipLaunchKernelGGL(k_scale_unless_one, dim3((unsigned)blocks), dim3(256), 0, stream, x, n,
                     d_scale);
  return check_launch("k_scale_unless_one");
}

int hgnn_uniform_i32(const uint64_t* d_seed, int64_t n, int32_t hi, int32_t* out,
                     hgnn_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  if (n < 0 || hi < 1) return fail(HGNN_E_ARG, "uniform_i32: n=%lld hi=%d", (long long)n, hi);
  if (n == 0) return HGNN_OK;
  if (!d_seed || !out) return fail(HGNN_E_ARG, "uniform_i32: null pointer");
  hipLaunchKernelGGL(k_uniform_i32, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, d_seed,
                     n, (uint32_t)hi, out);
  return check_launch("k_uniform_i32");
}

}  // extern "C"
