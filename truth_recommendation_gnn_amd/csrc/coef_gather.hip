// dP of the sampled-softmax link loss: hgnn_coef_gather2_planned (contract in include/hgnn.h).
//
//   dP[r] = sum_{p in positives of r} coef_pos[p] U[col[p]] + sum_{q in negatives of r} coef_neg[q] U[col_n[q]]
//
// The two-list planned gather of hgnn_score_gather2_planned_lq (gather.hip) with each pair's
// weight READ at the pair's position in its list instead of recomputed from <U[u], P[r]>: a
// softmax coefficient depends on all 1 + k logits of its edge, which the row's wave does not
// have, so the scoring pass (softmax_loss.hip) emits it and the negatives' sort carries it as a
// payload.  It reads no P rows and no logQ table.  Same items: a row's wave sums the lists that
// are not heavy; a list longer than `chunk` is summed chunk by chunk into a slab (the positives'
// by the static plan, the negatives' by the per-step device plan, waves beyond the device counts
// return at once) and added to the row by a fix-up in fixed order: the positives' partial sums,
// then the negatives'.  One write per row, no atomics, sums in the lists' stable order: two runs
// are bitwise equal.  U comes as fp32, bf16 or zero-packed fp32 rows (zpack.h; the lane reads of
// zpack_lanes.h, as the ZP score gather makes them).
#include "hgnn_common.h"
#include "zpack.h"
#include "zpack_lanes.h"

namespace hgnn {

struct CoefArgs {
  const void* x;               // U: fp32 rows, bf16 rows or zero-packed fp32 rows
  const int32_t* rowptr;       // the positives grouped by post, with the static plan below
  const int32_t* col;
  const float* coef;           // [E] by position of col
  const int32_t* rowptr2;      // the negatives grouped by post (this step's sort)
  const int32_t* col2;
  const float* coef2;          // [E k] by position of col2
  const int32_t* heavy_rows;
  const int32_t* heavy_first;
  float* slab;
  const int32_t* nheavy_rows;  // the negatives' plan, made on the device: [max_heavy]
  const int32_t* nheavy_first; // [max_heavy + 1]
  const int32_t* ncounts;      // device {n_heavy, n_chunks}
  float* nslab;                // [max_chunks * d]
  float* out;
  int64_t n_rows;
  int64_t n_heavy;
  int64_t n_items;             // rows + the positives' chunks
  int64_t max_heavy;
  int64_t max_chunks;
  int32_t d;
  int32_t chunk;
  int32_t nt_load;
  int32_t nt_store;
};

// Sum of coef[p] * x[col[p]] over [beg, end) into acc (per lane VPL vectors of width W; each slot
// of LPR lanes its own partial sum): segment_sum's weighted form, the weight of edge p loaded by
// the lane that loads col[p].
template <int LPR, int VPL, int W, int UNROLL, typename XT>
__device__ __forceinline__ void coef_segment(const CoefArgs& a, const int32_t* col,
                                             const float* coef, int64_t beg, int64_t end,
                                             typename Vec<W>::T (&acc)[VPL]) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  constexpr int NS = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, sl = lane % LPR;
  const int d = a.d;
  for (int64_t base = beg; base < end; base += 64) {
    const int n = (int)min<int64_t>(64, end - base);
    int cidx = 0;
    float wv = 0.f;
    if (lane < n) {
      cidx = col[base + lane];
      wv = coef[base + lane];
    }
    for (int j = 0; j < n; j += NS * UNROLL) {
      typename S::Raw v[UNROLL][VPL];
      float we[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int e = j + u * NS + slot;
        const int src = __shfl(cidx, e & 63, 64);
        we[u] = __shfl(wv, e & 63, 64);
        const XT* xr = static_cast<const XT*>(a.x) + (int64_t)src * d;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int c = (q * LPR + sl) * W;
          if (a.nt_load) v[u][q] = (e < n && c < d) ? S::load_nt(xr + c) : S::zero();
          else v[u][q] = (e < n && c < d) ? S::load(xr + c) : S::zero();
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int q = 0; q < VPL; ++q) V::fma(acc[q], we[u], S::widen(v[u][q]));
    }
  }
}

// coef_segment over zero-packed rows (fp32, one float4 per lane: d = 64 or 128): segment_sum_zp's
// loads (per row a lane's mask word and 16 B of values at an offset taken from the mask, both
// unconditional; an edge slot past the segment's end reads row 0 with its nibble forced to 0; the
// next round's masks requested right after this round's values) with the weights read a batch
// ahead as the ids are.
template <int LPR, int UNROLL, bool NT>
__device__ __forceinline__ void coef_segment_zp(const CoefArgs& a, const int32_t* col,
                                                const float* coef, int64_t beg, int64_t end,
                                                float4& acc) {
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
  float widx = lane < end - beg ? coef[beg + lane] : 0.f;
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
    const float wnext = lane < left ? coef[base + 64 + lane] : 0.f;
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
      float we[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) we[u] = __shfl(widx, (j + u * NS + slot) & 63, 64);
      const bool same = j + R < n;            // (wave-uniform) the next round is in this batch
      const int csel = same ? cidx : cnext;
      const int j0 = same ? j + R : 0;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        src[u] = __shfl(csel, (j0 + u * NS + slot) & 63, 64);
        m[u] = MK::load(xb + (int64_t)src[u] * S, sl);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        uint32_t c[4];
        zpack::expand(t[u].x, t[u].y, t[u].z, t[u].w, nib[u], c);
        const float4 v = make_float4(__uint_as_float(c[0]), __uint_as_float(c[1]),
                                     __uint_as_float(c[2]), __uint_as_float(c[3]));
        V::fma(acc, we[u], v);
      }
    }
    cidx = cnext;
    widx = wnext;
  }
}

// item: a row, a chunk of a row heavy in its positives (slab), or a chunk of a row heavy in its
// negatives (nslab), in that order (gather_item_pn's)
template <int LPR, int VPL, int W, int UNROLL, typename XT, int ZP>
__device__ __forceinline__ void coef_item(const CoefArgs& a, const int64_t item) {
  using V = Vec<W>;
  const int lane = threadIdx.x & 63;
  const int sl = lane % LPR;
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
    int64_t lo = 0, hi = a.n_heavy;             // heavy_first[h] <= slot < heavy_first[h + 1]
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
    const int64_t n_heavy = min<int64_t>(a.ncounts[0], a.max_heavy);
    if (slot >= min<int64_t>(a.ncounts[1], a.max_chunks) || n_heavy < 1) return;
    int64_t lo = 0, hi = n_heavy;
    while (hi - lo > 1) {
      int64_t mid = (lo + hi) >> 1;
      if (a.nheavy_first[mid] <= slot) lo = mid; else hi = mid;
    }
    row = a.nheavy_rows[lo];
    beg2 = a.rowptr2[row] + (slot - a.nheavy_first[lo]) * a.chunk;
    end2 = min<int64_t>(beg2 + a.chunk, a.rowptr2[row + 1]);
    dst = a.nslab + slot * a.d;
  }
  typename V::T acc[VPL];
#pragma unroll
  for (int q = 0; q < VPL; ++q) acc[q] = V::zero();
  if constexpr (ZP != 0) {
    static_assert(VPL == 1 && W == 4 && sizeof(XT) == 4, "zero-packed rows: fp32, d = 64 / 128");
    coef_segment_zp<LPR, UNROLL, ZP == 2>(a, a.col, a.coef, beg, end, acc[0]);
    coef_segment_zp<LPR, UNROLL, ZP == 2>(a, a.col2, a.coef2, beg2, end2, acc[0]);
  } else {
    coef_segment<LPR, VPL, W, UNROLL, XT>(a, a.col, a.coef, beg, end, acc);
    coef_segment<LPR, VPL, W, UNROLL, XT>(a, a.col2, a.coef2, beg2, end2, acc);
  }
  // combine the NS slots (lanes sl, sl + LPR, ...); the first slot writes
#pragma unroll
  for (int m = LPR; m < 64; m <<= 1)
#pragma unroll
    for (int q = 0; q < VPL; ++q) V::add(acc[q], V::shfl_xor(acc[q], m));
  if (lane >= LPR) return;
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    const int c = (q * LPR + sl) * W;
    if (c < a.d) {
      if (a.nt_store) V::store_nt(dst + c, acc[q]);
      else V::store(dst + c, acc[q]);
    }
  }
}

template <int LPR, int VPL, int W, int UNROLL, typename XT>
__global__ void __launch_bounds__(256) k_coef_gather(const CoefArgs a) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items + a.max_chunks) return;
  coef_item<LPR, VPL, W, UNROLL, XT, 0>(a, item);
}

// (the register budget of k_gather_pn_zp: a round's loaded words and the next round's masks)
template <int LPR, int UNROLL, int ZP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
k_coef_gather_zp(const CoefArgs a) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items + a.max_chunks) return;
  coef_item<LPR, 1, 4, UNROLL, float, ZP>(a, item);
}

// out[row] += sum_k slab[first + k] for the heavy rows of one plan: k_fixup_neg's slices and
// fixed-order LDS tree, one block per (possible) heavy row.  counts: the device-side {n_heavy,
// n_chunks} of the negatives' plan (blocks beyond them return), or null for the static plan.
template <int W>
__global__ void __launch_bounds__(256) k_coef_fixup(const float* slab, const int32_t* heavy_rows,
                                                    const int32_t* heavy_first,
                                                    const int32_t* counts, int64_t max_heavy,
                                                    int64_t max_chunks, float* out, int32_t d) {
  using V = Vec<W>;
  __shared__ typename V::T buf[256];
  const int64_t h = blockIdx.x;
  if (counts && h >= min<int64_t>(counts[0], max_heavy)) return;   // (uniform over the block)
  const int64_t row = heavy_rows[h];
  const int64_t f0 = heavy_first[h];
  const int64_t f1 = min<int64_t>(heavy_first[h + 1], max_chunks);
  const int nvec = (d + W - 1) / W;
  int cpb = 1;
  while (cpb < nvec && cpb < 256) cpb <<= 1;
  const int S = 256 / cpb;
  const int slice = threadIdx.x / cpb, cv = threadIdx.x % cpb;
  for (int c0 = 0; c0 < nvec; c0 += cpb) {
    const int c = (c0 + cv) * W;
    typename V::T r = V::zero();
    if (c < d)
      for (int64_t k = f0 + slice; k < f1; k += S) V::add(r, V::load(slab + k * d + c));
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
    if (slice == 0 && c < d) {
      typename V::T t = buf[threadIdx.x];
      float* o = out + row * d + c;
      V::add(t, V::load(o));
      V::store(o, t);
    }
    __syncthreads();
  }
}

template <typename XT, int LPR, int VPL, int W, int UNROLL>
static int launch_coef(const CoefArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((k_coef_gather<LPR, VPL, W, UNROLL, XT>), grid, dim3(256), 0, stream, a);
  return check_launch(sizeof(XT) == 2 ? "k_coef_gather(bf16)" : "k_coef_gather");
}

// the lane layouts and depths of the weighted gathers of gather.hip's width tables
static int launch_coef_f32(const CoefArgs& a, dim3 grid, hipStream_t s) {
  const int d = a.d;
  if (d % 4 == 0) {
    const int nv = d / 4;
    if (nv <= 4) return launch_coef<float, 4, 1, 4, 4>(a, grid, s);
    if (nv <= 8) return launch_coef<float, 8, 1, 4, 4>(a, grid, s);
    if (nv <= 16) return launch_coef<float, 16, 1, 4, 6>(a, grid, s);
    if (nv <= 32) return launch_coef<float, 32, 1, 4, 4>(a, grid, s);
    if (nv <= 64) return launch_coef<float, 64, 1, 4, 4>(a, grid, s);
    if (nv <= 128) return launch_coef<float, 64, 2, 4, 2>(a, grid, s);
    if (nv <= 256) return launch_coef<float, 64, 4, 4, 2>(a, grid, s);
  } else {
    if (d <= 16) return launch_coef<float, 16, 1, 1, 4>(a, grid, s);
    if (d <= 64) return launch_coef<float, 64, 1, 1, 4>(a, grid, s);
    if (d <= 256) return launch_coef<float, 64, 4, 1, 2>(a, grid, s);
    if (d <= 1024) return launch_coef<float, 64, 16, 1, 1>(a, grid, s);
  }
  return fail(HGNN_E_UNSUPPORTED, "coef_gather2_planned: d=%d > 1024", d);
}

static int launch_coef_bf16(const CoefArgs& a, dim3 grid, hipStream_t s) {
  using B = uint16_t;
  const int nv = a.d / 8;
  if (nv <= 2) return launch_coef<B, 2, 1, 8, 2>(a, grid, s);
  if (nv <= 4) return launch_coef<B, 4, 1, 8, 4>(a, grid, s);
  if (nv <= 8) return launch_coef<B, 8, 1, 8, 3>(a, grid, s);
  if (nv <= 16) return launch_coef<B, 16, 1, 8, 2>(a, grid, s);
  if (nv <= 32) return launch_coef<B, 32, 1, 8, 4>(a, grid, s);
  if (nv <= 64) return launch_coef<B, 64, 1, 8, 4>(a, grid, s);
  return launch_coef<B, 64, 2, 8, 2>(a, grid, s);
}

static int launch_coef_zp(const CoefArgs& a, dim3 grid, hipStream_t stream) {
#define HGNN_CZP(LPR, ZP) \
  hipLaunchKernelGGL((k_coef_gather_zp<LPR, 4, ZP>), grid, dim3(256), 0, stream, a)
  if (a.d == 64) {
    if (a.nt_load) HGNN_CZP(16, 2); else HGNN_CZP(16, 1);
  } else {
    if (a.nt_load) HGNN_CZP(32, 2); else HGNN_CZP(32, 1);
  }
#undef HGNN_CZP
  return check_launch("k_coef_gather(zp)");
}

// the score gathers' policy (gather.hip, kNtBytes): a table of at least 1 GiB is streamed with nt
// loads and the output rows are then stored nt too (a zero-packed table counts unpacked)
constexpr int64_t kCoefNtBytes = int64_t(1) << 30;

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_coef_gather2_planned(int32_t rows, const void* x, int64_t n_x, int32_t d,
                              const int32_t* rowptr, const int32_t* col, const float* coef_pos,
                              const int32_t* rowptr_n, const int32_t* col_n,
                              const float* coef_neg, int64_t n_rows, const int32_t* heavy_rows,
                              const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                              int32_t chunk, float* slab, const int32_t* neg_heavy_rows,
                              const int32_t* neg_heavy_first, const int32_t* d_neg_counts2,
                              int64_t neg_max_heavy, float* neg_slab, float* out,
                              hgnn_stream_t stream_) {
  const char* who = "coef_gather2_planned";
  hipStream_t stream = as_stream(stream_);
  if (rows < HGNN_ROWS_F32 || rows > HGNN_ROWS_ZP) return fail(HGNN_E_ARG, "%s: rows=%d", who, rows);
  if (d <= 0 || n_rows < 0 || n_x < 0 || n_heavy < 0 || n_chunks < 0 || chunk <= 0 ||
      neg_max_heavy < 0)
    return fail(HGNN_E_ARG, "%s: bad sizes d=%d n_rows=%lld chunk=%d", who, d, (long long)n_rows,
                chunk);
  if (rows == HGNN_ROWS_BF16 && (d % 8 != 0 || d > 1024))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (bf16 rows need d %% 8 == 0 and d <= 1024)", who, d);
  if (rows == HGNN_ROWS_ZP && !zpack::width_ok(d))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (zero-packed rows: 64 or 128)", who, d);
  if (rows == HGNN_ROWS_F32 && d > 1024) return fail(HGNN_E_UNSUPPORTED, "%s: d=%d > 1024", who, d);
  if (n_rows == 0) return HGNN_OK;
  // x / col / coef may be null only for lists without entries (nothing is dereferenced then)
  if (!rowptr || !rowptr_n || !out)
    return fail(HGNN_E_ARG, "%s: null rowptr / rowptr_n / out", who);
  if (n_heavy > 0 && (!heavy_rows || !heavy_first || !slab))
    return fail(HGNN_E_ARG, "%s: heavy rows without plan/slab", who);
  if (neg_max_heavy > 0 && (!neg_heavy_rows || !neg_heavy_first || !d_neg_counts2 || !neg_slab))
    return fail(HGNN_E_ARG, "%s: the negatives' plan has null arrays", who);
  CoefArgs a{};
  a.x = x; a.rowptr = rowptr; a.col = col; a.coef = coef_pos;
  a.rowptr2 = rowptr_n; a.col2 = col_n; a.coef2 = coef_neg;
  a.heavy_rows = heavy_rows; a.heavy_first = heavy_first; a.slab = slab;
  a.nheavy_rows = neg_heavy_rows; a.nheavy_first = neg_heavy_first; a.ncounts = d_neg_counts2;
  a.nslab = neg_slab; a.out = out;
  a.n_rows = n_rows; a.n_heavy = n_heavy; a.n_items = n_rows + (n_heavy > 0 ? n_chunks : 0);
  a.max_heavy = neg_max_heavy; a.max_chunks = 2 * neg_max_heavy;
  a.d = d; a.chunk = chunk;
  a.nt_load = n_x * d * (rows == HGNN_ROWS_BF16 ? 2 : 4) >= kCoefNtBytes ? 1 : 0;
  a.nt_store = a.nt_load;
  const dim3 grid((unsigned)cdiv(a.n_items + a.max_chunks, 4));
  int rc;
  if (rows == HGNN_ROWS_ZP) rc = launch_coef_zp(a, grid, stream);
  else if (rows == HGNN_ROWS_BF16) rc = launch_coef_bf16(a, grid, stream);
  else rc = launch_coef_f32(a, grid, stream);
  if (rc) return rc;
  // the fix-ups in a fixed order: the positives' partial sums, then the negatives'
  if (n_heavy > 0) {
    const dim3 fgrid((unsigned)n_heavy);
    if (d % 4 == 0)
      hipLaunchKernelGGL(k_coef_fixup<4>, fgrid, dim3(256), 0, stream, slab, heavy_rows,
                         heavy_first, nullptr, n_heavy, n_chunks, out, d);
    else
      hipLaunchKernelGGL(k_coef_fixup<1>, fgrid, dim3(256), 0, stream, slab, heavy_rows,
                         heavy_first, nullptr, n_heavy, n_chunks, out, d);
    if (int rc2 = check_launch("k_coef_fixup")) return rc2;
  }
  if (neg_max_heavy > 0) {
    const dim3 fgrid((unsigned)neg_max_heavy);
    if (d % 4 == 0)
      hipLaunchKernelGGL(k_coef_fixup<4>, fgrid, dim3(256), 0, stream, neg_slab, neg_heavy_rows,
                         neg_heavy_first, d_neg_counts2, neg_max_heavy, a.max_chunks, out, d);
    else
      hipLaunchKernelGGL(k_coef_fixup<1>, fgrid, dim3(256), 0, stream, neg_slab, neg_heavy_rows,
                         neg_heavy_first, d_neg_counts2, neg_max_heavy, a.max_chunks, out, d);
    return check_launch("k_coef_fixup(neg)");
  }
  return HGNN_OK;
}

}  // extern "C"
