// K1 / K2: segmented gather-reduce over a CSR — the E x d heart of SAGE mean aggregation.
//
//   out[i,:] (+)= s_i * sum_{p in row i} w_p * x[col[p], :]
//
// HBM-bound (algorithmic bytes per edge: 4 B index + 4*d B source row [+ 4 B weight]).
// Mapping (wave64, one item per wave):
//   * a row of d floats is read by LPR lanes, 16 B (float4) per lane and VPL vectors per lane,
//     so a wave covers NS = 64/LPR rows per load instruction (d=64: 4 rows x 256 B = 1 KiB);
//   * the wave pulls 64 column indices (and weights) of its row with one coalesced load, then
//     each slot of LPR lanes takes every NS-th edge, UNROLL rows in flight per slot;
//   * slots are combined with xor-shuffles; the first slot writes the row (full 256-B lines).
// No atomics: each destination row is owned by one wave, so sums are deterministic.  Rows longer
// than `chunk` edges (power-law heads) are split by the plan into chunk-sized items whose
// partial sums go to a slab, then k_fixup adds them in chunk order.
//
// Score mode (the link loss's dP): an edge's weight is its BCE coefficient, recomputed from the
// score with bce_terms.h's helpers as the scoring pass forms it (scoring.hip): a positive's
// sigma(s) - 1 as -sigma(-s) (pos_coef_t), a negative's sigma(s), in every instantiation -- plain,
// weighted, zero-packed, planned, with or without the logQ offset.
#include "hgnn_common.h"
#include "zpack.h"
#include "zpack_lanes.h"

// Cache policy of the gathered rows and the output rows (set per launch from the table sizes,
// `nt_policy` / `hot_policy` below): nt loads / stores when the table is far larger than the
// caches; with a col_hot, nt loads for all but the relation's most referenced rows.
#include <stdlib.h>
#include <string.h>

namespace hgnn {

struct GatherArgs {
  const void* x;               // source table: fp32 rows, or bf16 rows when `bf16` is set
  const int32_t* rowptr;
  const int32_t* col;
  const float* edge_w;
  const float* col_w;
  const float* row_w;          // per-row output scale (replaces the mean's 1/segment length)
  const int32_t* heavy_rows;
  const int32_t* heavy_first;
  float* slab;
  float* out;
  int64_t n_rows;
  int64_t n_heavy;
  int64_t n_items;
  int32_t d;
  int32_t chunk;
  int32_t mean;
  int32_t accumulate;
  int64_t acc_limit;           // > 0: only rows below it accumulate, the others are written
                               // fresh (a K2 whose output holds a root-gradient prefix)
  // score mode (hgnn_score_gather): w_p = f(<x[col[p]], rowvec[row]>) recomputed per edge
  const void* rowvec;          // (of the source table's element type)
  const float* cscale;
  float inv_e;
  int32_t score;               // 1: -c*inv_e*sigmoid(-s)   2: inv_e*sigmoid(s)
  // hgnn_score_gather2: a second grouped list (the negatives, mode 2, no heavy-row plan) summed
  // into the same rows in the same pass; null otherwise
  const int32_t* rowptr2;
  int32_t nt_load;             // rows gathered with nt loads (score gathers over multi-GB tables)
  int32_t nt_store;            // output rows stored with nt stores
  const int32_t* col2;
  int32_t hot;                 // col holds hot flags in bit 31 (hgnn_hot_cols): two-policy loads
  int32_t bf16;                // x (and rowvec) hold bf16 rows: the XT = uint16_t instantiations
  int32_t zp;                  // x holds zero-packed fp32 rows (zpack.h): the ZP instantiations
  // the LQ instantiations (hgnn_score_gather2_lq): the logit of an edge of row r is its score less
  // row_bias[r], for both lists; null otherwise
  const float* row_bias;
};

// bit 31 of a col_hot entry: the source row is one of the relation's H most referenced rows
constexpr int32_t kHotIdMask = 0x7fffffff;

// segment_sum over zero-packed source rows (score mode, fp32, one float4 per lane: d = 64 or
// 128).  The lane layout, the edges of a round and every sum are segment_sum's: lane sl of a
// slot owns columns 4 sl .. 4 sl + 3, and what it feeds to the dot product and the fmas is the
// unpacked row's float4 bit for bit (zpack::expand), so the result is bitwise the same.
//
// Per row a lane makes two loads, both unconditional: its mask word (ZpMask) and 16 B of values
// at an offset taken from the mask (nt where the unpacked kernel's row loads are).  An edge slot
// past the segment's end reads row 0 (col of an idle lane is 0) with its nibble forced to 0; an
// offset is in the slot for any mask (zpack.h).  The masks of the next round (of the next
// 64-edge batch after a batch's last round) are requested right after this round's values, so
// the mask -> value dependency is exposed once per item, not once per round.
//
// EW (the first list of hgnn_score_gather2_w_zp): the edge's weight edge_w[p] is loaded by the
// lane that loads col[p], a batch ahead as cnext is (widx / wnext), and is shuffled to its slot
// where the round's weights are formed, so no round holds a register per row for it; the order
// of the mask and value loads is unchanged.
//
// LQ: the row's offset rb (one scalar per item, loaded by gather_item beside rv) is subtracted
// from each dot product before the sigmoid; nothing else moves.
template <int LPR, int UNROLL, bool NT, bool EW = false, bool LQ = false>
__device__ __forceinline__ void segment_sum_zp(const GatherArgs& a, const int32_t* col, int score,
                                               int64_t beg, int64_t end, const float4& rv,
                                               float4& acc, float rb = 0.f) {
  using V = Vec<4>;
  using MK = ZpMask<LPR>;
  constexpr int NS = 64 / LPR;
  constexpr int R = NS * UNROLL;   // edges per round
  static_assert(64 % R == 0, "a round never crosses a 64-edge batch");
  if (beg >= end) return;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, sl = lane % LPR;
  const char* xb = static_cast<const char*>(a.x);
  const int64_t S = zpack::slot_bytes(a.d);
  int cidx = lane < end - beg ? col[beg + lane] : 0;
  float widx = 0.f;
  if constexpr (EW) widx = lane < end - beg ? a.edge_w[beg + lane] : 0.f;
  uint32_t m[UNROLL];
  int src[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    src[u] = __shfl(cidx, u * NS + slot, 64);
    m[u] = MK::load(xb + (int64_t)src[u] * S, sl);
  }
  for (int64_t base = beg; base < end; base += 64) {
    const int n = (int)min<int64_t>(64, end - base);
    const int64_t left = end - base - 64;   // edges of the batches after this one
    const int cnext = lane < left ? col[base + 64 + lane] : 0;
    float wnext = 0.f;
    if constexpr (EW) wnext = lane < left ? a.edge_w[base + 64 + lane] : 0.f;
    for (int j = 0; j < n; j += R) {
      uint4 t[UNROLL];
      uint32_t nib[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int e = j + u * NS + slot;
        const zpack::LaneRead L = MK::read(m[u], sl);
        nib[u] = e < n ? L.nib : 0u;
        t[u] = zp_load16<NT>(xb + (int64_t)src[u] * S + zpack::value_byte(L.pre));
      }
      const bool same = j + R < n;            // (wave-uniform) the next round is in this batch
      const int csel = same ? cidx : cnext;
      const int j0 = same ? j + R : 0;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        src[u] = __shfl(csel, (j0 + u * NS + slot) & 63, 64);
        m[u] = MK::load(xb + (int64_t)src[u] * S, sl);
      }
      float4 v[UNROLL];
      float we[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        uint32_t c[4];
        zpack::expand(t[u].x, t[u].y, t[u].z, t[u].w, nib[u], c);
        v[u] = make_float4(__uint_as_float(c[0]), __uint_as_float(c[1]), __uint_as_float(c[2]),
                           __uint_as_float(c[3]));
      }
      const float cw = score == 1 ? *a.cscale * a.inv_e : a.inv_e;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        float sdot = 0.f;
        sdot += V::dot(rv, v[u]);
        sdot = slot_sum<LPR>(sdot);
        if constexpr (LQ) sdot -= rb;
        // (segment_sum's weights: pos_coef_t for the positives, mode 1)
        const float tt = exp_neg_abs(sdot);
        if constexpr (EW)   // (the weighted list is the positives')
          we[u] = cw * __shfl(widx, (j + u * NS + slot) & 63, 64) * pos_coef_t(sdot, tt);
        else
          we[u] = cw * pair_coef_t(score == 1, sdot, tt);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) V::fma(acc, we[u], v[u]);
    }
    cidx = cnext;
    if constexpr (EW) widx = wnext;
  }
}

// Sum of row segment [beg, end) of `col` into acc (per lane: VPL vectors of width W; each slot of
// LPR lanes holds its own partial sum, combined by slot_combine).  SC: the weight of each edge is
// recomputed from the score <x[col[p]], rv> (rv = the row's own vector, e.g. P[post] for the loss
// gradient dP) with weight mode `score`, so no per-edge weight array is stored or read.
//
// HOT: `col` is a col_hot array.  A flagged (hot) row is read with the default policy and stays
// cacheable; every other row is read nt, so the long tail of rows referenced once or twice no
// longer pushes the Zipf head out of L2 and the Infinity Cache.  The flag is uniform per slot of
// LPR lanes; both loads of a vector sit in one diamond on it, issued before anything waits, as
// the bounds-predicated load of the plain kernel is (ISA: the UNROLL rows' loads, then one
// s_waitcnt vmcnt(0), in both kernels).
//
// HAS_W with SC (the first list of hgnn_score_gather2_w): the recomputed weight is scaled by the
// edge's own, w(s) = c * inv_e * edge_w[p] * (sigmoid(s) - 1), read at the absolute position p as
// col is, so a heavy row's chunks need nothing new.
//
// XT: the source table's element type (RowSrc).  A bf16 row is read 16 B per lane, so d = 128 is
// 16 lanes per row and 4 rows per wave load; its vectors stay packed while in flight and are
// widened to fp32 where they are summed.  Everything after the load is fp32 either way.
//
// LQ with SC (hgnn_score_gather2_lq): the logit is the score less rb, the row's own offset
// (row_bias[row], loaded once per item by gather_item), for either weight mode; the weights'
// expressions are those of the other instantiations.
template <int LPR, int VPL, int W, int UNROLL, bool HAS_W, bool SC, bool HOT, typename XT = float,
          int ZP = 0, bool LQ = false>
__device__ __forceinline__ void segment_sum(const GatherArgs& a, const int32_t* col, int score,
                                            int64_t beg, int64_t end,
                                            const typename Vec<W>::T (&rv)[VPL],
                                            typename Vec<W>::T (&acc)[VPL], float rb = 0.f) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  if constexpr (ZP != 0) {
    static_assert(SC && !HOT && VPL == 1 && W == 4 && sizeof(XT) == 4,
                  "zero-packed rows: the fp32 score gather at d = 64 / 128");
    segment_sum_zp<LPR, UNROLL, ZP == 2, HAS_W, LQ>(a, col, score, beg, end, rv[0], acc[0], rb);
    return;
  }
  constexpr int NS = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, sl = lane % LPR;
  const int d = a.d;
  for (int64_t base = beg; base < end; base += 64) {
    const int n = (int)min<int64_t>(64, end - base);
    int cidx = 0;
    float wv = 1.f;
    if (lane < n) {
      cidx = col[base + lane];
      if (HAS_W) {
        wv = a.edge_w ? a.edge_w[base + lane] : 1.f;
        if (a.col_w) wv *= a.col_w[HOT ? cidx & kHotIdMask : cidx];
      }
    }
    for (int j = 0; j < n; j += NS * UNROLL) {
      typename S::Raw v[UNROLL][VPL];
      float we[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int e = j + u * NS + slot;
        const int raw = __shfl(cidx, e & 63, 64);
        const int src = HOT ? raw & kHotIdMask : raw;
        const bool cold = HOT && raw >= 0;
        we[u] = HAS_W ? __shfl(wv, e & 63, 64) : 1.f;
        const XT* xr = static_cast<const XT*>(a.x) + (int64_t)src * d;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int c = (q * LPR + sl) * W;
          // the dP score gather over a multi-GB user table streams its rows with nt loads (cfg4:
          // 32.4 -> 31.0 ms; on a table the Infinity Cache half holds, cfg3, 2.80 -> 3.42 ms, so
          // only above 1 GiB); the mean gathers keep the default policy (nt costs them 25-45 %:
          // the source-block passes and the Zipf-hot post rows live on cache reuse)
          if (SC && a.nt_load)
            v[u][q] = (e < n && c < d) ? S::load_nt(xr + c) : S::zero();
          else if (HOT)
            v[u][q] = (e < n && c < d) ? (cold ? S::load_nt(xr + c) : S::load(xr + c)) : S::zero();
          else
            v[u][q] = (e < n && c < d) ? S::load(xr + c) : S::zero();
        }
      }
      if constexpr (SC) {
        const float cw = score == 1 ? *a.cscale * a.inv_e : a.inv_e;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          float sdot = 0.f;
#pragma unroll
          for (int q = 0; q < VPL; ++q) sdot += V::dot(rv[q], S::widen(v[u][q]));
          sdot = slot_sum<LPR>(sdot);
          if constexpr (LQ) sdot -= rb;
          // the positives' sigmoid(z) - 1 formed as -sigmoid(-z) (pos_coef_t: the same t, no
          // cancellation): from z ~ 17 up 1/(1 + t) - 1 is exactly 0 in fp32
          const float tt = exp_neg_abs(sdot);
          if constexpr (HAS_W) we[u] = cw * we[u] * pos_coef_t(sdot, tt);   // (mode 1)
          else we[u] = cw * pair_coef_t(score == 1, sdot, tt);
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          if (HAS_W || SC) V::fma(acc[q], we[u], S::widen(v[u][q]));
          else V::add(acc[q], S::widen(v[u][q]));
        }
    }
  }
}

// combine the NS slots (lanes sl, sl+LPR, ...)
template <int LPR, int VPL, int W>
__device__ __forceinline__ void slot_combine(typename Vec<W>::T (&acc)[VPL]) {
  using V = Vec<W>;
#pragma unroll
  for (int m = LPR; m < 64; m <<= 1)
#pragma unroll
    for (int q = 0; q < VPL; ++q) V::add(acc[q], V::shfl_xor(acc[q], m));
}

// one item (a light row, or a chunk of a heavy row) per wave
template <int LPR, int VPL, int W, int UNROLL, bool HAS_W, bool SC, bool HOT = false,
          typename XT = float, int ZP = 0, bool LQ = false>
__device__ __forceinline__ void gather_item(const GatherArgs& a, const int64_t item) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  const int lane = threadIdx.x & 63;
  const int sl = lane % LPR;
  const bool writer = lane < LPR;
  int64_t row, beg, end;
  float* dst;
  bool partial;
  const bool two = SC && a.rowptr2;             // hgnn_score_gather2: + the negatives' segment
  bool own = true;                              // this wave sums the row's (first) segment
  if (item < a.n_rows) {                       // light row: whole row in this wave
    row = item;
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
    if (end - beg > a.chunk) {                  // heavy: handled by chunks + fixup ...
      if (!two) return;
      own = false;                              // ... the second list's segment still here
    }
    dst = a.out + row * a.d;
    partial = false;
  } else {                                      // chunk of a heavy row -> slab slot
    const int64_t slot = item - a.n_rows;
    int64_t lo = 0, hi = a.n_heavy;             // heavy_first[h] <= slot < heavy_first[h+1]
    while (hi - lo > 1) {
      int64_t mid = (lo + hi) >> 1;
      if (a.heavy_first[mid] <= slot) lo = mid; else hi = mid;
    }
    row = a.heavy_rows[lo];
    const int64_t k = slot - a.heavy_first[lo];
    beg = a.rowptr[row] + k * a.chunk;
    end = min<int64_t>(beg + a.chunk, a.rowptr[row + 1]);
    dst = a.slab + slot * a.d;
    partial = true;
  }
  typename V::T acc[VPL], rv[VPL];
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    acc[q] = V::zero();
    const int c = (q * LPR + sl) * W;
    rv[q] = (SC && c < a.d)
                ? S::widen(S::load(static_cast<const XT*>(a.rowvec) + row * a.d + c))
                : V::zero();
  }
  float rb = 0.f;   // LQ: the row's offset, one scalar per item beside its rv
  if constexpr (LQ) rb = a.row_bias[row];
  if (own)
    segment_sum<LPR, VPL, W, UNROLL, HAS_W, SC, HOT, XT, ZP, LQ>(a, a.col, a.score, beg, end, rv,
                                                                 acc, rb);
  // (the second list carries no per-edge weights: HAS_W stays off for it in a score gather)
  if (two && !partial)
    segment_sum<LPR, VPL, W, UNROLL, HAS_W && !SC, SC, false, XT, ZP, LQ>(
        a, a.col2, 2, a.rowptr2[row], a.rowptr2[row + 1], rv, acc, rb);
  slot_combine<LPR, VPL, W>(acc);
  if (!writer) return;
  float s = 1.f;
  if (!partial) {
    if (a.row_w) s = a.row_w[row];
    else if (a.mean) s = end > beg ? 1.f / (float)(end - beg) : 0.f;
  }
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    const int c = (q * LPR + sl) * W;
    if (c < a.d) {
      typename V::T r = acc[q];
      if (!partial) {
        V::scale(r, s);
        if (a.accumulate && (a.acc_limit == 0 || row < a.acc_limit)) V::add(r, V::load(dst + c));
      }
      if (a.nt_store) V::store_nt(dst + c, r);
      else V::store(dst + c, r);
    }
  }
}

template <int LPR, int VPL, int W, int UNROLL, bool HAS_W, bool SC = false, bool HOT = false,
          typename XT = float, bool LQ = false>
__global__ void __launch_bounds__(256) k_gather(const GatherArgs a) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items) return;
  gather_item<LPR, VPL, W, UNROLL, HAS_W, SC, HOT, XT, 0, LQ>(a, item);
}

// The ZP gather as its own kernel (ZP = 1, or 2 with nt value loads): it holds a round's loaded
// words and the next round's masks at once, and left to itself the register allocator spent
// 112 VGPRs on it (4 waves per SIMD); asked for 6 waves it fits without a spill in the loop.
template <int LPR, int UNROLL, int ZP, bool EW = false, bool LQ = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
k_gather_zp(const GatherArgs a) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items) return;
  gather_item<LPR, 1, 4, UNROLL, EW, true, false, float, ZP, LQ>(a, item);
}

// Several gathers of one row width in one launch (hgnn_gather_reduce_multi): job j owns the
// waves [base[j], base[j + 1]); light rows only (no heavy-row plan), distinct outputs.
constexpr int kGatherMultiMax = 8;
struct GatherMulti {
  GatherArgs j[kGatherMultiMax];
  int64_t base[kGatherMultiMax + 1];
  int32_t n;
};

template <int LPR, int VPL, int W, int UNROLL, bool HAS_W>
__global__ void __launch_bounds__(256) k_gather_multi(const GatherMulti m) {
  // the wave index made scalar: the job search and the job's arguments are then scalar loads
  // (a per-lane index fetched every argument with vector loads, one more dependent round trip
  // per wave — slower than the separate launches)
  const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= m.base[m.n]) return;
  int j = 0;
  while (j + 1 < m.n && item >= m.base[j + 1]) ++j;
  gather_item<LPR, VPL, W, UNROLL, HAS_W, false>(m.j[j], item - m.base[j]);
}

// Heavy rows: out[row] (+)= s * sum_k slab[first + k].  One block per heavy row: S slices of
// the chunk list (strided) x the row's vectors, then a fixed-order LDS tree => deterministic.
template <int W>
__global__ void __launch_bounds__(256) k_fixup(const GatherArgs a) {
  using V = Vec<W>;
  __shared__ typename V::T buf[256];
  const int64_t h = blockIdx.x;
  const int64_t row = a.heavy_rows[h];
  const int64_t f0 = a.heavy_first[h], f1 = a.heavy_first[h + 1];
  const int64_t deg = a.rowptr[row + 1] - a.rowptr[row];
  const float s = a.row_w ? a.row_w[row] : (a.mean ? (deg > 0 ? 1.f / (float)deg : 0.f) : 1.f);
  const int nvec = (a.d + W - 1) / W;
  int cpb = 1;
  while (cpb < nvec && cpb < 256) cpb <<= 1;
  const int S = 256 / cpb;
  const int slice = threadIdx.x / cpb, cv = threadIdx.x % cpb;
  for (int c0 = 0; c0 < nvec; c0 += cpb) {
    const int c = (c0 + cv) * W;
    typename V::T r = V::zero();
    if (c < a.d) {
      int64_t k = f0 + slice;
      for (; k + 3 * S < f1; k += 4 * S) {   // 4 independent loads in flight
        typename V::T x0 = V::load(a.slab + k * a.d + c);
        typename V::T x1 = V::load(a.slab + (k + S) * a.d + c);
        typename V::T x2 = V::load(a.slab + (k + 2 * S) * a.d + c);
        typename V::T x3 = V::load(a.slab + (k + 3 * S) * a.d + c);
        V::add(x0, x1); V::add(x2, x3); V::add(x0, x2); V::add(r, x0);
      }
      for (; k < f1; k += S) V::add(r, V::load(a.slab + k * a.d + c));
    }
    buf[threadIdx.x] = r;
    __syncthreads();
    for (int st = S / 2; st >= 1; st >>= 1) {
      if (slice < st) {
        typename V::T t = buf[threadIdx.x];
        V::add(t, buf[threadIdx.x + st * cpb]);
        buf[threadIdx.x] = t;
      }
      __syncthreads();
    }
    if (slice == 0 && c < a.d) {
      typename V::T t = buf[threadIdx.x];
      V::scale(t, s);
      float* o = a.out + row * a.d + c;
      if ((a.accumulate && (a.acc_limit == 0 || row < a.acc_limit)) || a.rowptr2)
        V::add(t, V::load(o));
      V::store(o, t);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- planned negatives (skewed)
// hgnn_score_gather2_planned: the two-list score gather whose second list (the negatives) has a
// heavy-row plan of its own.  Negatives drawn in proportion to popularity put a post's share of
// all E k draws into its list, which k_gather would sum whole in the row's one wave.  Here a list
// longer than `chunk` is summed chunk by chunk into a second slab, one wave per chunk with the
// same segment_sum in mode 2; the row's own wave skips it, and k_fixup_neg adds the partial sums
// to the row in chunk order after k_fixup has added the positives'.  The negatives change every
// step, so their plan is made on the device (hgnn_plan_device) and nothing about it is known to
// the host: the arrays and the grid are sized by the bound that the pair count gives, the counts
// are read from device memory, and the waves and blocks beyond them return at once.
// The kernels above are not touched: these are instantiations of their own.
struct NegPlan {
  const int32_t* heavy_rows;    // [max_heavy]
  const int32_t* heavy_first;   // [max_heavy + 1]
  const int32_t* counts;        // device {n_heavy, n_chunks}
  float* slab;                  // [max_chunks * d]
  int64_t max_heavy;
  int64_t max_chunks;
};

// item: a row, a chunk of a row heavy in its positives (slab), or a chunk of a row heavy in its
// negatives (NegPlan::slab), in that order
template <int LPR, int VPL, int W, int UNROLL, bool HAS_W, typename XT, int ZP, bool LQ = false>
__device__ __forceinline__ void gather_item_pn(const GatherArgs& a, const NegPlan& p,
                                               const int64_t item) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  const int lane = threadIdx.x & 63;
  const int sl = lane % LPR;
  const bool writer = lane < LPR;
  int64_t row, beg = 0, end = 0, beg2 = 0, end2 = 0;
  float* dst;
  if (item < a.n_rows) {                        // a row: the lists that are not heavy
    row = item;
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
    if (end - beg > a.chunk) end = beg;
    beg2 = a.rowptr2[row];
    end2 = a.rowptr2[row + 1];
    if (end2 - beg2 > a.chunk) end2 = beg2;
    dst = a.out + row * a.d;
  } else if (item < a.n_items) {                // chunk of a row heavy in its positives
    const int64_t slot = item - a.n_rows;
    int64_t lo = 0, hi = a.n_heavy;
    while (hi - lo > 1) {
      int64_t mid = (lo + hi) >> 1;
      if (a.heavy_first[mid] <= slot) lo = mid; else hi = mid;
    }
    row = a.heavy_rows[lo];
    beg = a.rowptr[row] + (slot - a.heavy_first[lo]) * a.chunk;
    end = min<int64_t>(beg + a.chunk, a.rowptr[row + 1]);
    dst = a.slab + slot * a.d;
  } else {                                      // chunk of a row heavy in its negatives
    const int64_t slot = item - a.n_items;
    const int64_t n_heavy = min<int64_t>(p.counts[0], p.max_heavy);
    if (slot >= min<int64_t>(p.counts[1], p.max_chunks) || n_heavy < 1) return;
    int64_t lo = 0, hi = n_heavy;
    while (hi - lo > 1) {
      int64_t mid = (lo + hi) >> 1;
      if (p.heavy_first[mid] <= slot) lo = mid; else hi = mid;
    }
    row = p.heavy_rows[lo];
    beg2 = a.rowptr2[row] + (slot - p.heavy_first[lo]) * a.chunk;
    end2 = min<int64_t>(beg2 + a.chunk, a.rowptr2[row + 1]);
    dst = p.slab + slot * a.d;
  }
  typename V::T acc[VPL], rv[VPL];
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    acc[q] = V::zero();
    const int c = (q * LPR + sl) * W;
    rv[q] = c < a.d ? S::widen(S::load(static_cast<const XT*>(a.rowvec) + row * a.d + c))
                    : V::zero();
  }
  float rb = 0.f;   // LQ: the row's offset, for whichever list (or chunk of one) this item sums
  if constexpr (LQ) rb = a.row_bias[row];
  segment_sum<LPR, VPL, W, UNROLL, HAS_W, true, false, XT, ZP, LQ>(a, a.col, 1, beg, end, rv, acc,
                                                                   rb);
  segment_sum<LPR, VPL, W, UNROLL, false, true, false, XT, ZP, LQ>(a, a.col2, 2, beg2, end2, rv,
                                                                   acc, rb);
  slot_combine<LPR, VPL, W>(acc);
  if (!writer) return;
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    const int c = (q * LPR + sl) * W;
    if (c < a.d) {
      if (a.nt_store) V::store_nt(dst + c, acc[q]);
      else V::store(dst + c, acc[q]);
    }
  }
}

template <int LPR, int VPL, int W, int UNROLL, bool HAS_W, typename XT, bool LQ = false>
__global__ void __launch_bounds__(256) k_gather_pn(const GatherArgs a, const NegPlan p) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items + p.max_chunks) return;
  gather_item_pn<LPR, VPL, W, UNROLL, HAS_W, XT, 0, LQ>(a, p, item);
}

template <int LPR, int UNROLL, int ZP, bool EW, bool LQ = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
k_gather_pn_zp(const GatherArgs a, const NegPlan p) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items + p.max_chunks) return;
  gather_item_pn<LPR, 1, 4, UNROLL, EW, float, ZP, LQ>(a, p, item);
}

// out[row] += sum_k slab[first + k] for the rows heavy in their negatives: k_fixup's slices and
// fixed-order LDS tree, one block per possible heavy row (those beyond the device count return)
template <int W>
__global__ void __launch_bounds__(256) k_fixup_neg(const GatherArgs a, const NegPlan p) {
  using V = Vec<W>;
  __shared__ typename V::T buf[256];
  const int64_t h = blockIdx.x;
  if (h >= min<int64_t>(p.counts[0], p.max_heavy)) return;   // (uniform over the block)
  const int64_t row = p.heavy_rows[h];
  const int64_t f0 = p.heavy_first[h];
  const int64_t f1 = min<int64_t>(p.heavy_first[h + 1], p.max_chunks);
  const int nvec = (a.d + W - 1) / W;
  int cpb = 1;
  while (cpb < nvec && cpb < 256) cpb <<= 1;
  const int S = 256 / cpb;
  const int slice = threadIdx.x / cpb, cv = threadIdx.x % cpb;
  for (int c0 = 0; c0 < nvec; c0 += cpb) {
    const int c = (c0 + cv) * W;
    typename V::T r = V::zero();
    if (c < a.d)
      for (int64_t k = f0 + slice; k < f1; k += S) V::add(r, V::load(p.slab + k * a.d + c));
    buf[threadIdx.x] = r;
    __syncthreads();
    for (int st = S / 2; st >= 1; st >>= 1) {
      if (slice < st) {
        typename V::T t = buf[threadIdx.x];
        V::add(t, buf[threadIdx.x + st * cpb]);
        buf[threadIdx.x] = t;
      }
      __syncthreads();
    }
    if (slice == 0 && c < a.d) {
      typename V::T t = buf[threadIdx.x];
      float* o = a.out + row * a.d + c;
      V::add(t, V::load(o));
      V::store(o, t);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------- host half
// Every entry point is its own argument rules, gather_args (+ score_args / hot_args), run_gather;
// run_gather validates, derives the Variant once and launches from the element type's width table.
enum class Variant { kScore, kScoreWeighted, kHotWeighted, kHot, kWeighted, kPlain };

// One row of a width table: the lane layout and the rows in flight per slot (the depth) per
// variant: UM the mean / plain sum, UW weighted, US the score gather.
template <int LPR_, int VPL_, int W_, int UM_, int UW_, int US_>
struct Shape {
  static constexpr int LPR = LPR_, VPL = VPL_, W = W_, UM = UM_, UW = UW_, US = US_;
};

// The fp32 row widths: f(Shape) for the row that takes d (k_gather and k_gather_multi).
template <typename F>
static int with_shape_f32(int d, F&& f) {
  if (d % 4 == 0) {
    const int nv = d / 4;  // float4 vectors per row
    if (nv <= 4) return f(Shape<4, 1, 4, 4, 4, 4>{});
    if (nv <= 8) return f(Shape<8, 1, 4, 4, 4, 4>{});
    // d = 64: rows in flight per wave (4 x the depth) chosen per variant on cfg2 (MI355X).  The
    // mean gathers take 32: user rows average 20 edges, so one round of loads covers most of
    // them (user<-post 0.84 -> 0.80 ms); the weighted K2 24 (0.50 -> 0.485 ms); the score
    // gather keeps 16 (its dot products hold more registers: 1.39 ms at 16, 1.50 at 32).
    if (nv <= 16) return f(Shape<16, 1, 4, 8, 6, 4>{});
    // d = 128 (512-B rows): 8, 12 or 16 rows in flight measured the same on cfg3 and cfg4; 8
    // kept (the 12- and 16-deep forms are no longer built)
    if (nv <= 32) return f(Shape<32, 1, 4, 4, 4, 4>{});
    if (nv <= 64) return f(Shape<64, 1, 4, 4, 4, 4>{});
    if (nv <= 128) return f(Shape<64, 2, 4, 2, 2, 2>{});
    if (nv <= 256) return f(Shape<64, 4, 4, 2, 2, 2>{});
  } else {
    if (d <= 16) return f(Shape<16, 1, 1, 4, 4, 4>{});
    if (d <= 64) return f(Shape<64, 1, 1, 4, 4, 4>{});
    if (d <= 256) return f(Shape<64, 4, 1, 2, 2, 2>{});
    if (d <= 1024) return f(Shape<64, 16, 1, 1, 1, 1>{});
  }
  return fail(HGNN_E_UNSUPPORTED, "gather: d=%d > 1024", d);
}

// bf16 source rows (W = 8, 16 B per lane; d % 8 == 0 and d <= 1024, bf16_width_rule).
// The depths are the fp32 kernels' rows in flight at the same d (d = 64: 32 / 24 / 16 rows,
// d = 128: 8).  At d = 128 twice that (16 rows, the fp32 kernel's BYTES in flight) measured the
// same at cfg4 (K1 post<-user 7.64 - 7.77 ms at 8 rows, 7.58 - 7.59 at 16; the dP gather 15.73 -
// 15.99 against 15.68 - 16.28; the step 89.7 - 90.0 against 89.0 - 90.1 ms): 8 kept, the form
// with fewer registers held; the deeper one is no longer built.
template <typename F>
static int with_shape_bf16(int d, F&& f) {
  const int nv = d / 8;  // 16-B vectors per row
  if (nv <= 2) return f(Shape<2, 1, 8, 2, 2, 2>{});
  if (nv <= 4) return f(Shape<4, 1, 8, 4, 4, 4>{});
  if (nv <= 8) return f(Shape<8, 1, 8, 4, 3, 2>{});
  if (nv <= 16) return f(Shape<16, 1, 8, 2, 2, 2>{});
  if (nv <= 32) return f(Shape<32, 1, 8, 4, 4, 4>{});
  if (nv <= 64) return f(Shape<64, 1, 8, 4, 4, 4>{});
  return f(Shape<64, 2, 8, 2, 2, 2>{});
}

// The six variants of one table row over XT rows (float, or uint16_t for bf16).
template <typename XT, int LPR, int VPL, int W, int UM, int UW, int US>
static int launch_gather(Shape<LPR, VPL, W, UM, UW, US>, const GatherArgs& a, Variant v,
                         hipStream_t stream) {
  const dim3 grid((unsigned)cdiv(a.n_items, 4)), block(256);
#define HGNN_G(U, HAS_W, SC, HOT) \
  hipLaunchKernelGGL((k_gather<LPR, VPL, W, U, HAS_W, SC, HOT, XT>), grid, block, 0, stream, a)
  if (a.row_bias) {   // the LQ instantiations: the two score variants alone (run_gather's rule)
    if (v == Variant::kScoreWeighted)
      hipLaunchKernelGGL((k_gather<LPR, VPL, W, US, true, true, false, XT, true>), grid, block, 0,
                         stream, a);
    else
      hipLaunchKernelGGL((k_gather<LPR, VPL, W, US, false, true, false, XT, true>), grid, block, 0,
                         stream, a);
    return check_launch(sizeof(XT) == 2 ? "k_gather(lq, bf16)" : "k_gather(lq)");
  }
  switch (v) {
    case Variant::kScore: HGNN_G(US, false, true, false); break;
    case Variant::kScoreWeighted: HGNN_G(US, true, true, false); break;   // per-edge weights
    // the two-policy loads as their own instantiations (hot_policy)
    case Variant::kHotWeighted: HGNN_G(UW, true, false, true); break;
    case Variant::kHot: HGNN_G(UM, false, false, true); break;
    case Variant::kWeighted: HGNN_G(UW, true, false, false); break;
    case Variant::kPlain: HGNN_G(UM, false, false, false); break;
  }
#undef HGNN_G
  return check_launch(sizeof(XT) == 2 ? "k_gather(bf16)" : "k_gather");
}

// zero-packed source rows: the score gather's d = 64 / d = 128 forms (their lane layouts and
// depths), nothing else (run_score2 alone sets GatherArgs::zp, after its width rule)
static int launch_gather_zp(const GatherArgs& a, Variant v, hipStream_t stream) {
  const dim3 grid((unsigned)cdiv(a.n_items, 4)), block(256);
#define HGNN_GZP(LPR, ZP)                                                                      \
  do {                                                                                         \
    if (a.row_bias && v == Variant::kScoreWeighted)                                            \
      hipLaunchKernelGGL((k_gather_zp<LPR, 4, ZP, true, true>), grid, block, 0, stream, a);    \
    else if (a.row_bias)                                                                       \
      hipLaunchKernelGGL((k_gather_zp<LPR, 4, ZP, false, true>), grid, block, 0, stream, a);   \
    else if (v == Variant::kScoreWeighted)                                                     \
      hipLaunchKernelGGL((k_gather_zp<LPR, 4, ZP, true>), grid, block, 0, stream, a);          \
    else                                                                                       \
      hipLaunchKernelGGL((k_gather_zp<LPR, 4, ZP>), grid, block, 0, stream, a);                \
  } while (0)
  if (a.d == 64) {
    if (a.nt_load) HGNN_GZP(16, 2); else HGNN_GZP(16, 1);
  } else {
    if (a.nt_load) HGNN_GZP(32, 2); else HGNN_GZP(32, 1);
  }
#undef HGNN_GZP
  return check_launch("k_gather(zp)");
}

// nt above 1 GiB: cfg4's 4.6 GB user table and its 4.6 GB user-side outputs.  Output rows of
// the dP gather / K2s / means are read by another kernel long after they left L2 (cfg4 step
// 168.1 -> 167.5 ms with nt stores, mostly the dP gather); cfg2/cfg3 tables stay cache-resident.
constexpr int64_t kNtBytes = int64_t(1) << 30;
// The rule itself (hgnn_gather_nt_policy): a score gather streams the rows of a source table of
// at least kNtBytes and then stores its rows nt too; any other gather stores nt where its output
// is that large.
static void gather_nt_policy(int64_t n_x, int32_t d, int64_t elem, bool score, int64_t n_rows,
                             int32_t* nt_load, int32_t* nt_store) {
  *nt_load = score && n_x * d * elem >= kNtBytes ? 1 : 0;
  *nt_store = (score ? *nt_load != 0 : n_rows * d * 4 >= kNtBytes) ? 1 : 0;
}
// (`elem`: bytes per element of the source table, so the threshold sees the table's real size;
// the output rows are fp32 either way)
static void nt_policy(GatherArgs& a, int64_t n_x, int64_t elem = 4) {
  gather_nt_policy(n_x, a.d, elem, a.score != 0, a.n_rows, &a.nt_load, &a.nt_store);
}
// (a zero-packed table counts by its unpacked size: the policy of hgnn_score_gather2)
static int64_t elem_bytes(const GatherArgs& a) { return a.bf16 ? 2 : 4; }

// Two-policy loads (col_hot): on when the table outgrows the Infinity Cache (the scoring pass's
// nt_neg threshold), the caller passed a col_hot, and the flagged rows carry at least half of
// the edges.  Measured at cfg4 (512-MB post table, Zipf(0.8) ids, K1 / K2 user<-post, policy off
// 11.49 / 11.63 ms): flagging the 32768 .. 131072 most referenced rows (48 - 65 % of the edges)
// gives 10.70 - 10.88 / 10.87 - 11.03 ms, 16384 rows (41 %) 11.03 / 11.21, 8192 rows (35 %) no
// gain and 4096 rows (29 %) a loss (12.05 / 12.23): an nt row loses the Infinity Cache as well
// as L2, so the cold set must be the tail that neither cache would have kept.  Below half of the
// edges the rule keeps the old kernel.  HGNN_HOT_ROWS=0 turns the policy off,
// HGNN_HOT_ROWS=force on for any table that comes with a col_hot (tests).  Read per call: a
// getenv against a 10-ms kernel.
constexpr int64_t kHotTableBytes = int64_t(256) << 20;
constexpr float kHotShareMin = 0.5f;
static bool hot_policy(int64_t table_bytes, bool has_col_hot, float hot_share) {
  if (!has_col_hot) return false;
  const char* e = getenv("HGNN_HOT_ROWS");
  if (e && !strcmp(e, "0")) return false;
  if (e && !strcmp(e, "force")) return true;
  return table_bytes >= kHotTableBytes && hot_share >= kHotShareMin;
}

// The fields every gather has: table, grouping, weights, flags, heavy-row plan, slab, out.
static GatherArgs gather_args(const void* x, int32_t d, const int32_t* rowptr, const int32_t* col,
                              int64_t n_rows, const float* edge_w, const float* col_w,
                              const float* row_w, int32_t flags, int64_t acc_limit,
                              const int32_t* heavy_rows, const int32_t* heavy_first,
                              int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                              float* out) {
  GatherArgs a{};
  a.x = x; a.rowptr = rowptr; a.col = col; a.edge_w = edge_w; a.col_w = col_w; a.row_w = row_w;
  a.heavy_rows = heavy_rows; a.heavy_first = heavy_first; a.slab = slab; a.out = out;
  a.n_rows = n_rows; a.n_heavy = n_heavy; a.n_items = n_rows + (n_heavy > 0 ? n_chunks : 0);
  a.d = d; a.chunk = chunk; a.mean = (flags & HGNN_MEAN) ? 1 : 0;
  a.accumulate = (flags & HGNN_ACCUMULATE) ? 1 : 0;
  a.acc_limit = acc_limit;
  return a;
}

// score mode: the row's own vectors and the weight mode; optionally the second grouped list
static void score_args(GatherArgs& a, const void* rowvec, const float* cscale, float inv_e,
                       int32_t mode, const int32_t* rowptr2 = nullptr,
                       const int32_t* col2 = nullptr) {
  a.rowvec = rowvec; a.cscale = cscale; a.inv_e = inv_e; a.score = mode;
  a.rowptr2 = rowptr2; a.col2 = col2;
}

// the two-policy loads, where hot_policy wants them: the flagged ids replace col
static void hot_args(GatherArgs& a, int64_t n_x, const int32_t* col_hot, float hot_share) {
  if (hot_policy(n_x * (int64_t)a.d * elem_bytes(a), col_hot != nullptr, hot_share)) {
    a.col = col_hot;
    a.hot = 1;
  }
}

// Argument rules that several entry points share, each worded with the entry's name (`who`).
static int bf16_width_rule(int32_t d, const char* who) {
  if (d <= 0 || (d % 8 == 0 && d <= 1024)) return HGNN_OK;   // (d <= 0: run_gather's bad sizes)
  return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (bf16 rows need d %% 8 == 0 and d <= 1024)", who, d);
}
static int acc_limit_rule(int64_t acc_limit, const char* who, int job = -1) {
  if (acc_limit >= 0) return HGNN_OK;
  if (job >= 0) return fail(HGNN_E_ARG, "%s: acc_limit[%d] < 0", who, job);
  return fail(HGNN_E_ARG, "%s: acc_limit < 0", who);
}
static int row_w_rule(const float* row_w, int32_t flags, const char* who) {
  if (!row_w || !(flags & HGNN_MEAN)) return HGNN_OK;
  return fail(HGNN_E_ARG, "%s: row_w replaces HGNN_MEAN, not both", who);
}

// `n_x`: rows of the source table (the cache policy of the launch, nt_policy)
static int run_gather(GatherArgs a, int64_t n_x, hipStream_t stream) {
  nt_policy(a, n_x, elem_bytes(a));
  if (a.d <= 0 || a.n_rows < 0 || a.n_heavy < 0 || a.chunk <= 0)
    return fail(HGNN_E_ARG, "gather: bad sizes d=%d n_rows=%lld chunk=%d", a.d,
                (long long)a.n_rows, a.chunk);
  if (a.n_rows == 0) return HGNN_OK;
  // x / col may be null only for a CSR without edges (nothing is dereferenced then)
  if (!a.rowptr || !a.out) return fail(HGNN_E_ARG, "gather: null rowptr/out");
  if (a.n_heavy > 0 && (!a.heavy_rows || !a.heavy_first || !a.slab))
    return fail(HGNN_E_ARG, "gather: heavy rows without plan/slab");
  const bool has_w = a.edge_w || a.col_w;
  // a score gather's only weights: edge_w on the positives (mode 1) of a two-list gather
  const bool score_w = a.score == 1 && a.rowptr2 && a.edge_w && !a.col_w;
  if (a.score && ((has_w && !score_w) || a.mean || !a.rowvec || (a.score == 1 && !a.cscale)))
    return fail(HGNN_E_ARG, "score_gather: bad mode/arguments");
  if (a.rowptr2 && a.score != 1)
    return fail(HGNN_E_ARG, "score_gather2: needs mode 1 for the first list");
  if (a.row_bias && !(a.score == 1 && a.rowptr2))
    return fail(HGNN_E_ARG, "gather: row_bias belongs to the two-list score gather");
  const Variant v = a.score ? (score_w ? Variant::kScoreWeighted : Variant::kScore)
                    : a.hot ? (has_w ? Variant::kHotWeighted : Variant::kHot)
                            : (has_w ? Variant::kWeighted : Variant::kPlain);
  int rc;
  if (a.zp)
    rc = launch_gather_zp(a, v, stream);
  else if (a.bf16)
    rc = with_shape_bf16(a.d, [&](auto s) { return launch_gather<uint16_t>(s, a, v, stream); });
  else
    rc = with_shape_f32(a.d, [&](auto s) { return launch_gather<float>(s, a, v, stream); });
  if (rc) return rc;
  if (a.n_heavy > 0) {
    const dim3 grid((unsigned)a.n_heavy), block(256);
    if (a.d % 4 == 0) hipLaunchKernelGGL(k_fixup<4>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_fixup<1>, grid, block, 0, stream, a);
    return check_launch("k_fixup");
  }
  return HGNN_OK;
}

// The two-list score gathers: mode 1 over (rowptr, col) with the heavy-row plan, the negatives
// (rowptr_n, col_n) in mode 2, one write per row; x holds fp32, bf16 or zero-packed fp32 rows.
// `weighted`: the _w entries, whose positives carry edge_w (per position of rowptr / col).
enum class Rows { kF32, kBf16, kZp };
static int run_score2(const char* who, Rows rows, const void* x, int64_t n_x, const void* rowvec,
                      int32_t d, const int32_t* rowptr, const int32_t* col,
                      const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                      const float* cscale, float inv_e, const int32_t* heavy_rows,
                      const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks, int32_t chunk,
                      float* slab, float* out, hgnn_stream_t stream, bool weighted = false,
                      const float* edge_w = nullptr, const float* row_bias = nullptr) {
  if (rows == Rows::kBf16)
    if (int rc = bf16_width_rule(d, who)) return rc;
  if (rows == Rows::kZp && !zpack::width_ok(d))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (zero-packed rows: 64 or 128)", who, d);
  if (!rowptr_n && n_rows > 0) return fail(HGNN_E_ARG, "%s: rowptr_n is null", who);
  if (weighted && !edge_w && n_rows > 0) return fail(HGNN_E_ARG, "%s: edge_w is null", who);
  GatherArgs a = gather_args(x, d, rowptr, col, n_rows, edge_w, nullptr, nullptr, 0, 0,
                             heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, out);
  score_args(a, rowvec, cscale, inv_e, 1, rowptr_n, col_n);
  a.bf16 = rows == Rows::kBf16;
  a.zp = rows == Rows::kZp;
  a.row_bias = row_bias;
  return run_gather(a, n_x, as_stream(stream));
}

// The planned form's launches: the score gather of the element type's width table (per-edge
// weights or not), then the two fix-ups in a fixed order.
template <typename XT, int LPR, int VPL, int W, int UM, int UW, int US>
static int launch_gather_pn(Shape<LPR, VPL, W, UM, UW, US>, const GatherArgs& a, const NegPlan& p,
                            bool weighted, dim3 grid, hipStream_t stream) {
  if (a.row_bias) {   // the LQ instantiations
    if (weighted)
      hipLaunchKernelGGL((k_gather_pn<LPR, VPL, W, US, true, XT, true>), grid, dim3(256), 0,
                         stream, a, p);
    else
      hipLaunchKernelGGL((k_gather_pn<LPR, VPL, W, US, false, XT, true>), grid, dim3(256), 0,
                         stream, a, p);
    return check_launch(sizeof(XT) == 2 ? "k_gather_pn(lq, bf16)" : "k_gather_pn(lq)");
  }
  if (weighted)
    hipLaunchKernelGGL((k_gather_pn<LPR, VPL, W, US, true, XT>), grid, dim3(256), 0, stream, a, p);
  else
    hipLaunchKernelGGL((k_gather_pn<LPR, VPL, W, US, false, XT>), grid, dim3(256), 0, stream, a, p);
  return check_launch(sizeof(XT) == 2 ? "k_gather_pn(bf16)" : "k_gather_pn");
}

static int launch_gather_pn_zp(const GatherArgs& a, const NegPlan& p, bool weighted, dim3 grid,
                               hipStream_t stream) {
#define HGNN_GPZ(LPR, ZP)                                                                       \
  do {                                                                                          \
    if (a.row_bias && weighted)                                                                 \
      hipLaunchKernelGGL((k_gather_pn_zp<LPR, 4, ZP, true, true>), grid, dim3(256), 0, stream,  \
                         a, p);                                                                 \
    else if (a.row_bias)                                                                        \
      hipLaunchKernelGGL((k_gather_pn_zp<LPR, 4, ZP, false, true>), grid, dim3(256), 0, stream, \
                         a, p);                                                                 \
    else if (weighted)                                                                          \
      hipLaunchKernelGGL((k_gather_pn_zp<LPR, 4, ZP, true>), grid, dim3(256), 0, stream, a, p); \
    else                                                                                        \
      hipLaunchKernelGGL((k_gather_pn_zp<LPR, 4, ZP, false>), grid, dim3(256), 0, stream, a, p);\
  } while (0)
  if (a.d == 64) {
    if (a.nt_load) HGNN_GPZ(16, 2); else HGNN_GPZ(16, 1);
  } else {
    if (a.nt_load) HGNN_GPZ(32, 2); else HGNN_GPZ(32, 1);
  }
#undef HGNN_GPZ
  return check_launch("k_gather_pn(zp)");
}

static int run_score2_planned(Rows rows, const void* x, int64_t n_x, const void* rowvec, int32_t d,
                              const int32_t* rowptr, const int32_t* col, const float* edge_w,
                              const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                              const float* cscale, float inv_e, const int32_t* heavy_rows,
                              const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                              int32_t chunk, float* slab, NegPlan p, float* out,
                              hipStream_t stream, const char* who = "score_gather2_planned",
                              const float* row_bias = nullptr) {
  if (d <= 0 || n_rows < 0 || n_heavy < 0 || chunk <= 0 || p.max_heavy < 0)
    return fail(HGNN_E_ARG, "%s: bad sizes d=%d n_rows=%lld chunk=%d", who, d, (long long)n_rows,
                chunk);
  if (rows == Rows::kBf16)
    if (int rc = bf16_width_rule(d, who)) return rc;
  if (rows == Rows::kZp && !zpack::width_ok(d))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (zero-packed rows: 64 or 128)", who, d);
  if (n_rows == 0) return HGNN_OK;
  if (!rowptr || !rowptr_n || !rowvec || !cscale || !out)
    return fail(HGNN_E_ARG, "%s: null rowptr / rowptr_n / rowvec / cscale / out", who);
  if (n_heavy > 0 && (!heavy_rows || !heavy_first || !slab))
    return fail(HGNN_E_ARG, "%s: heavy rows without plan/slab", who);
  if (p.max_heavy > 0 && (!p.heavy_rows || !p.heavy_first || !p.counts || !p.slab))
    return fail(HGNN_E_ARG, "%s: the negatives' plan has null arrays", who);
  GatherArgs a = gather_args(x, d, rowptr, col, n_rows, edge_w, nullptr, nullptr, 0, 0,
                             heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, out);
  score_args(a, rowvec, cscale, inv_e, 1, rowptr_n, col_n);
  a.bf16 = rows == Rows::kBf16;
  a.zp = rows == Rows::kZp;
  a.row_bias = row_bias;
  nt_policy(a, n_x, elem_bytes(a));
  const bool weighted = edge_w != nullptr;
  const dim3 grid((unsigned)cdiv(a.n_items + p.max_chunks, 4));
  int rc;
  if (a.zp)
    rc = launch_gather_pn_zp(a, p, weighted, grid, stream);
  else if (a.bf16)
    rc = with_shape_bf16(d, [&](auto s) {
      return launch_gather_pn<uint16_t>(s, a, p, weighted, grid, stream);
    });
  else
    rc = with_shape_f32(d, [&](auto s) {
      return launch_gather_pn<float>(s, a, p, weighted, grid, stream);
    });
  if (rc) return rc;
  // the fix-ups in a fixed order: the positives' partial sums, then the negatives'
  if (a.n_heavy > 0) {
    const dim3 fgrid((unsigned)a.n_heavy);
    if (d % 4 == 0) hipLaunchKernelGGL(k_fixup<4>, fgrid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_fixup<1>, fgrid, dim3(256), 0, stream, a);
    if (int rc2 = check_launch("k_fixup")) return rc2;
  }
  if (p.max_heavy > 0) {
    const dim3 fgrid((unsigned)p.max_heavy);
    if (d % 4 == 0) hipLaunchKernelGGL(k_fixup_neg<4>, fgrid, dim3(256), 0, stream, a, p);
    else hipLaunchKernelGGL(k_fixup_neg<1>, fgrid, dim3(256), 0, stream, a, p);
    return check_launch("k_fixup_neg");
  }
  return HGNN_OK;
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_gather_reduce(const float* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                       const int32_t* col, int64_t n_rows, const float* edge_w,
                       const float* col_w, int32_t flags, const int32_t* heavy_rows,
                       const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                       int32_t chunk, float* slab, float* out, hgnn_stream_t stream) {
  return run_gather(gather_args(x, d, rowptr, col, n_rows, edge_w, col_w, nullptr, flags, 0,
                                heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, out),
                    n_x, as_stream(stream));
}

int32_t hgnn_hot_rows_policy(int64_t table_bytes, int32_t has_col_hot, float hot_share) {
  return hot_policy(table_bytes, has_col_hot != 0, hot_share) ? 1 : 0;
}

int32_t hgnn_gather_nt_policy(int64_t n_x, int32_t d, int32_t elem_bytes, int32_t score,
                              int64_t n_rows, int32_t* nt_load, int32_t* nt_store) {
  if (d < 1 || n_x < 0 || n_rows < 0 || (elem_bytes != 2 && elem_bytes != 4) || !nt_load ||
      !nt_store)
    return fail(HGNN_E_ARG, "gather_nt_policy: n_x=%lld d=%d elem_bytes=%d n_rows=%lld",
                (long long)n_x, d, elem_bytes, (long long)n_rows);
  gather_nt_policy(n_x, d, elem_bytes, score != 0, n_rows, nt_load, nt_store);
  return HGNN_OK;
}

int hgnn_gather_reduce_hot(const float* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                           const int32_t* col, int64_t n_rows, const float* edge_w,
                           const float* col_w, int32_t flags, const int32_t* heavy_rows,
                           const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                           int32_t chunk, float* slab, float* out, int64_t acc_limit,
                           const int32_t* col_hot, float hot_share, hgnn_stream_t stream) {
  if (int rc = acc_limit_rule(acc_limit, "gather_reduce_hot")) return rc;
  GatherArgs a = gather_args(x, d, rowptr, col, n_rows, edge_w, col_w, nullptr, flags, acc_limit,
                             heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, out);
  hot_args(a, n_x, col_hot, hot_share);
  return run_gather(a, n_x, as_stream(stream));
}

int hgnn_gather_reduce_multi(int32_t n_jobs, const float* const* x, const int64_t* n_x, int32_t d,
                             const int32_t* const* rowptr, const int32_t* const* col,
                             const int64_t* n_rows, const float* const* edge_w, int32_t flags,
                             const int64_t* acc_limit, float* const* out,
                             hgnn_stream_t stream_) {
  if (n_jobs < 1 || n_jobs > kGatherMultiMax || d <= 0 || d % 4 || d > 512)
    return fail(HGNN_E_ARG, "gather_reduce_multi: n_jobs=%d (1..%d) d=%d (4..512, % 4)", n_jobs,
                kGatherMultiMax, d);
  GatherMulti m{};
  m.n = n_jobs;
  bool has_w = false;
  for (int j = 0; j < n_jobs; ++j) {
    if (n_rows[j] < 0 || (n_rows[j] > 0 && (!rowptr[j] || !out[j])))
      return fail(HGNN_E_ARG, "gather_reduce_multi: job %d: null rowptr/out", j);
    for (int i = 0; i < j; ++i)
      if (n_rows[j] > 0 && out[i] == out[j])
        return fail(HGNN_E_ARG, "gather_reduce_multi: jobs %d and %d share an output", i, j);
    const int64_t limit = acc_limit ? acc_limit[j] : 0;
    if (int rc = acc_limit_rule(limit, "gather_reduce_multi", j)) return rc;
    // light rows only: no heavy-row plan, no row is ever split
    m.j[j] = gather_args(x[j], d, rowptr[j], col[j], n_rows[j], edge_w ? edge_w[j] : nullptr,
                         nullptr, nullptr, flags, limit, nullptr, nullptr, 0, 0, INT32_MAX,
                         nullptr, out[j]);
    has_w |= m.j[j].edge_w != nullptr;
    nt_policy(m.j[j], n_x[j]);
    m.base[j + 1] = m.base[j] + n_rows[j];
  }
  if (m.base[n_jobs] == 0) return HGNN_OK;
  const dim3 grid((unsigned)cdiv(m.base[n_jobs], 4)), block(256);
  hipStream_t stream = as_stream(stream_);
  // the rows of the fp32 table that the d rule above admits: float4 rows up to d = 512
  return with_shape_f32(d, [&](auto s) {
    using S = decltype(s);
    if constexpr (S::W == 4 && S::LPR * S::VPL * S::W <= 512) {
      if (has_w)
        hipLaunchKernelGGL((k_gather_multi<S::LPR, S::VPL, 4, S::UW, true>), grid, block, 0,
                           stream, m);
      else
        hipLaunchKernelGGL((k_gather_multi<S::LPR, S::VPL, 4, S::UM, false>), grid, block, 0,
                           stream, m);
      return check_launch("k_gather_multi");
    } else {
      return fail(HGNN_E_ARG, "gather_reduce_multi: no launch at d=%d", d);
    }
  });
}

int hgnn_gather_reduce_scaled(const float* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                              const int32_t* col, int64_t n_rows, const float* edge_w,
                              const float* col_w, const float* row_w, int32_t flags,
                              const int32_t* heavy_rows, const int32_t* heavy_first,
                              int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                              float* out, hgnn_stream_t stream) {
  if (int rc = row_w_rule(row_w, flags, "gather_reduce_scaled")) return rc;
  // (HGNN_MEAN is not read here: the scale is row_w, or 1 without one)
  return run_gather(gather_args(x, d, rowptr, col, n_rows, edge_w, col_w, row_w,
                                flags & ~HGNN_MEAN, 0, heavy_rows, heavy_first, n_heavy, n_chunks,
                                chunk, slab, out),
                    n_x, as_stream(stream));
}

int hgnn_gather_reduce_bf16(const uint16_t* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                            const int32_t* col, int64_t n_rows, const float* edge_w,
                            const float* col_w, const float* row_w, int32_t flags,
                            const int32_t* heavy_rows, const int32_t* heavy_first,
                            int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                            float* out, int64_t acc_limit, const int32_t* col_hot,
                            float hot_share, hgnn_stream_t stream) {
  if (int rc = bf16_width_rule(d, "gather_reduce_bf16")) return rc;
  if (int rc = row_w_rule(row_w, flags, "gather_reduce_bf16")) return rc;
  if (int rc = acc_limit_rule(acc_limit, "gather_reduce_bf16")) return rc;
  GatherArgs a = gather_args(x, d, rowptr, col, n_rows, edge_w, col_w, row_w, flags, acc_limit,
                             heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, out);
  a.bf16 = 1;
  hot_args(a, n_x, col_hot, hot_share);
  return run_gather(a, n_x, as_stream(stream));
}

int hgnn_gather_mean_fwd(const float* x_src, int64_t n_src, int32_t d, const int32_t* rowptr,
                         const int32_t* col, int64_t n_dst, const int32_t* heavy_rows,
                         const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                         int32_t chunk, float* slab, float* aggr, hgnn_stream_t stream) {
  return run_gather(gather_args(x_src, d, rowptr, col, n_dst, nullptr, nullptr, nullptr, HGNN_MEAN,
                                0, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, aggr),
                    n_src, as_stream(stream));
}

int hgnn_scatter_mean_bwd(const float* grad_aggr, int64_t n_dst, const float* inv_deg,
                          const int32_t* t_rowptr, const int32_t* t_col, int64_t n_src,
                          int32_t d, const int32_t* heavy_rows, const int32_t* heavy_first,
                          int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                          float* grad_x_src, int32_t accumulate, hgnn_stream_t stream) {
  if (!inv_deg && n_src > 0) return fail(HGNN_E_ARG, "scatter_mean_bwd: inv_deg is null");
  return run_gather(gather_args(grad_aggr, d, t_rowptr, t_col, n_src, nullptr, inv_deg, nullptr,
                                accumulate ? HGNN_ACCUMULATE : 0, 0, heavy_rows, heavy_first,
                                n_heavy, n_chunks, chunk, slab, grad_x_src),
                    n_dst, as_stream(stream));
}

int hgnn_score_gather(const float* x, int64_t n_x, const float* rowvec, int32_t d,
                      const int32_t* rowptr, const int32_t* col, int64_t n_rows, int32_t mode,
                      const float* cscale, float inv_e, const int32_t* heavy_rows,
                      const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                      int32_t chunk, float* slab, float* out, int32_t accumulate,
                      hgnn_stream_t stream) {
  if (mode != 1 && mode != 2) return fail(HGNN_E_ARG, "score_gather: mode=%d", mode);
  GatherArgs a = gather_args(x, d, rowptr, col, n_rows, nullptr, nullptr, nullptr,
                             accumulate ? HGNN_ACCUMULATE : 0, 0, heavy_rows, heavy_first, n_heavy,
                             n_chunks, chunk, slab, out);
  score_args(a, rowvec, cscale, inv_e, mode);
  return run_gather(a, n_x, as_stream(stream));
}

int hgnn_score_gather2(const float* x, int64_t n_x, const float* rowvec, int32_t d,
                       const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_n,
                       const int32_t* col_n, int64_t n_rows, const float* cscale, float inv_e,
                       const int32_t* heavy_rows, const int32_t* heavy_first, int64_t n_heavy,
                       int64_t n_chunks, int32_t chunk, float* slab, float* out,
                       hgnn_stream_t stream) {
  return run_score2("score_gather2", Rows::kF32, x, n_x, rowvec, d, rowptr, col, rowptr_n, col_n,
                    n_rows, cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab,
                    out, stream);
}

int hgnn_score_gather2_zp(const void* xz, int64_t n_x, const float* rowvec, int32_t d,
                          const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_n,
                          const int32_t* col_n, int64_t n_rows, const float* cscale, float inv_e,
                          const int32_t* heavy_rows, const int32_t* heavy_first, int64_t n_heavy,
                          int64_t n_chunks, int32_t chunk, float* slab, float* out,
                          hgnn_stream_t stream) {
  return run_score2("score_gather2_zp", Rows::kZp, xz, n_x, rowvec, d, rowptr, col, rowptr_n, col_n,
                    n_rows, cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab,
                    out, stream);
}

int hgnn_score_gather2_bf16(const uint16_t* x, int64_t n_x, const uint16_t* rowvec, int32_t d,
                            const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_n,
                            const int32_t* col_n, int64_t n_rows, const float* cscale,
                            float inv_e, const int32_t* heavy_rows, const int32_t* heavy_first,
                            int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                            float* out, hgnn_stream_t stream) {
  return run_score2("score_gather2_bf16", Rows::kBf16, x, n_x, rowvec, d, rowptr, col, rowptr_n,
                    col_n, n_rows, cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk,
                    slab, out, stream);
}

int hgnn_score_gather2_w(const float* x, int64_t n_x, const float* rowvec, int32_t d,
                         const int32_t* rowptr, const int32_t* col, const float* edge_w,
                         const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                         const float* cscale, float inv_e, const int32_t* heavy_rows,
                         const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                         int32_t chunk, float* slab, float* out, hgnn_stream_t stream) {
  return run_score2("score_gather2_w", Rows::kF32, x, n_x, rowvec, d, rowptr, col, rowptr_n, col_n,
                    n_rows, cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab,
                    out, stream, true, edge_w);
}

int hgnn_score_gather2_w_zp(const void* xz, int64_t n_x, const float* rowvec, int32_t d,
                            const int32_t* rowptr, const int32_t* col, const float* edge_w,
                            const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                            const float* cscale, float inv_e, const int32_t* heavy_rows,
                            const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                            int32_t chunk, float* slab, float* out, hgnn_stream_t stream) {
  return run_score2("score_gather2_w_zp", Rows::kZp, xz, n_x, rowvec, d, rowptr, col, rowptr_n,
                    col_n, n_rows, cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk,
                    slab, out, stream, true, edge_w);
}

int hgnn_score_gather2_w_bf16(const uint16_t* x, int64_t n_x, const uint16_t* rowvec, int32_t d,
                              const int32_t* rowptr, const int32_t* col, const float* edge_w,
                              const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                              const float* cscale, float inv_e, const int32_t* heavy_rows,
                              const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                              int32_t chunk, float* slab, float* out, hgnn_stream_t stream) {
  return run_score2("score_gather2_w_bf16", Rows::kBf16, x, n_x, rowvec, d, rowptr, col, rowptr_n,
                    col_n, n_rows, cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk,
                    slab, out, stream, true, edge_w);
}

int hgnn_score_gather2_planned(int32_t rows, const void* x, int64_t n_x, const void* rowvec,
                               int32_t d, const int32_t* rowptr, const int32_t* col,
                               const float* edge_w, const int32_t* rowptr_n, const int32_t* col_n,
                               int64_t n_rows, const float* cscale, float inv_e,
                               const int32_t* heavy_rows, const int32_t* heavy_first,
                               int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                               const int32_t* neg_heavy_rows, const int32_t* neg_heavy_first,
                               const int32_t* d_neg_counts2, int64_t neg_max_heavy,
                               float* neg_slab, float* out, hgnn_stream_t stream) {
  if (rows < HGNN_ROWS_F32 || rows > HGNN_ROWS_ZP)
    return fail(HGNN_E_ARG, "score_gather2_planned: rows=%d", rows);
  NegPlan p{};
  p.heavy_rows = neg_heavy_rows; p.heavy_first = neg_heavy_first; p.counts = d_neg_counts2;
  p.slab = neg_slab;
  p.max_heavy = neg_max_heavy;
  p.max_chunks = 2 * neg_max_heavy;
  const Rows r = rows == HGNN_ROWS_BF16 ? Rows::kBf16 : rows == HGNN_ROWS_ZP ? Rows::kZp : Rows::kF32;
  return run_score2_planned(r, x, n_x, rowvec, d, rowptr, col, edge_w, rowptr_n, col_n, n_rows,
                            cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab,
                            p, out, as_stream(stream));
}

int hgnn_score_gather2_lq(int32_t rows, const void* x, int64_t n_x, const void* rowvec, int32_t d,
                          const int32_t* rowptr, const int32_t* col, const float* edge_w,
                          const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                          const float* cscale, float inv_e, const float* row_bias,
                          const int32_t* heavy_rows, const int32_t* heavy_first, int64_t n_heavy,
                          int64_t n_chunks, int32_t chunk, float* slab, float* out,
                          hgnn_stream_t stream) {
  if (rows < HGNN_ROWS_F32 || rows > HGNN_ROWS_ZP)
    return fail(HGNN_E_ARG, "score_gather2_lq: rows=%d", rows);
  if (!row_bias) return fail(HGNN_E_ARG, "score_gather2_lq: row_bias is null");
  const Rows r = rows == HGNN_ROWS_BF16 ? Rows::kBf16 : rows == HGNN_ROWS_ZP ? Rows::kZp : Rows::kF32;
  return run_score2("score_gather2_lq", r, x, n_x, rowvec, d, rowptr, col, rowptr_n, col_n, n_rows,
                    cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab, out,
                    stream, false, edge_w, row_bias);
}

int hgnn_score_gather2_planned_lq(int32_t rows, const void* x, int64_t n_x, const void* rowvec,
                                  int32_t d, const int32_t* rowptr, const int32_t* col,
                                  const float* edge_w, const int32_t* rowptr_n,
                                  const int32_t* col_n, int64_t n_rows, const float* cscale,
                                  float inv_e, const float* row_bias, const int32_t* heavy_rows,
                                  const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                                  int32_t chunk, float* slab, const int32_t* neg_heavy_rows,
                                  const int32_t* neg_heavy_first, const int32_t* d_neg_counts2,
                                  int64_t neg_max_heavy, float* neg_slab, float* out,
                                  hgnn_stream_t stream) {
  const char* who = "score_gather2_planned_lq";
  if (rows < HGNN_ROWS_F32 || rows > HGNN_ROWS_ZP) return fail(HGNN_E_ARG, "%s: rows=%d", who, rows);
  if (!row_bias) return fail(HGNN_E_ARG, "%s: row_bias is null", who);
  NegPlan p{};
  p.heavy_rows = neg_heavy_rows; p.heavy_first = neg_heavy_first; p.counts = d_neg_counts2;
  p.slab = neg_slab;
  p.max_heavy = neg_max_heavy;
  p.max_chunks = 2 * neg_max_heavy;
  const Rows r = rows == HGNN_ROWS_BF16 ? Rows::kBf16 : rows == HGNN_ROWS_ZP ? Rows::kZp : Rows::kF32;
  return run_score2_planned(r, x, n_x, rowvec, d, rowptr, col, edge_w, rowptr_n, col_n, n_rows,
                            cscale, inv_e, heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab,
                            p, out, as_stream(stream), who, row_bias);
}

}  // extern "C"
