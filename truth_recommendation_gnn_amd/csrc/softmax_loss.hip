// Sampled-softmax (InfoNCE) link loss: the scoring pass (hgnn_edge_softmax_fwd; the contract is
// in include/hgnn.h, the scalar state of an edge in softmax_online.h).
//
//   z_j = <U[u], P[p_j]> / tau - b[p_j]        j = 0 (the positive) .. k
//   loss = sum_e g_e (logsumexp_j z_j - z_0)   g_e = c / E, or c w_e / E with per-edge weights
//
// A pair's gradient coefficient depends on all 1 + k logits of its edge, so the edge's rows are
// walked together.  The shape is the scoring pass's (scoring.hip, k_edge_score_k) with the loops
// exchanged: one wave per user keeps U[u] in registers, LPR lanes per row, NS = 64 / LPR slots;
// slot s takes edges s, s + NS, .. of a chunk of C positions (hgnn_softmax_chunk(k)) and walks
// each edge's rows 0 .. k in sequence, two rows per step through two register sets in ping-pong
// (a step may hold the last row of one edge and the first of the next).  Over an edge the slot
// carries the online-softmax state (m, l_neg), the positive's row and the row sum
//   a_e = sum_{j >= 1} exp(z_j - m) P[p_j]
// rescaled when the maximum moves; at the edge's last row G (a_e - l_neg P[p_0]) is folded into
// the wave's one dU accumulator, which is the edge's sum of coefficient x row with the positive's
// coefficient formed without cancellation (softmax_online.h).  Every post row is read once and
// dU[u] written once, no atomics but the out-of-range counter.
//
// The chunk's ids go through per-wave LDS at [position][column] with an odd stride (hardneg.hip's
// layout): the lanes load col and the chunk's C k contiguous negatives coalesced, check them once
// (an out-of-range id is counted into err, kept as -1 and given the offset +inf, which makes its
// logit -inf: it takes no part in the edge's softmax) and park each id beside its post's offset
// b[id].  A slot reads an id back where it loads the row and replaces the offset by the logit
// where it scores it.  After the chunk's rows the wave converts the parked logits with each
// edge's final (m, G) into the coefficients: coef_neg in the flat user-grouped order (the chunk's
// C k values are contiguous: coalesced stores), coef_pos by lane = position at slot_of[position].
//
// Loads of rows past the chunk, out-of-range ids and columns past d follow k_edge_score's
// unconditional-load convention: they read post 0 / column 0 and reach no result.
//
// LDS: (2 x 640 + 192) words x 4 waves x 4 B = 23 KiB per block; 6 blocks = 24 waves per CU fit
// 160 KiB.  All rows are read with plain loads (the hard-negative miner's finding for mined and
// popularity-weighted lists, the expected negatives here: their re-reads are worth keeping).
#include "hgnn_common.h"
#include "softmax_online.h"

namespace hgnn {

struct SoftmaxArgs {
  const void* U;               // fp32 rows, or bf16 rows in the XT = uint16_t instantiation
  const void* P;
  const int32_t* rowptr;       // user-grouped CSR of the positive edges
  const int32_t* col;          // positive post per position
  const int64_t* neg;          // [E, k] negatives in the user-grouped order, int64 ...
  const int32_t* neg32;        // ... or int32
  const float* edge_w;         // per-position weight of the edge, or null
  const float* post_bias;      // the logQ table b, or null (b = 0)
  const int32_t* slot_of;      // position -> index into coef_pos, or null (the position itself)
  const float* cscale;         // device scalar c
  float* dU;
  float* coef_pos;             // [E]
  float* coef_neg;             // [E, k], user-grouped order
  float* part;                 // [gridDim.x]
  int32_t* err;
  int64_t n_users;
  int64_t n_posts;
  float inv_e;
  float inv_tau;
  int32_t d, k, chunk;
  uint32_t magic;              // ceil(2^20 / k): r / k = (r * magic) >> 20 for r < 4096
};

template <int LPR, int VPL, int W, typename XT>
__global__ void __launch_bounds__(256) k_edge_softmax(const SoftmaxArgs a) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  using Raw = typename S::Raw;
  const XT* const Ux = static_cast<const XT*>(a.U);
  const XT* const Px = static_cast<const XT*>(a.P);
  constexpr int NS = 64 / LPR;
  __shared__ float s_z[4][softmax::kLdsWords];      // an entry's offset, then its logit
  __shared__ int32_t s_id[4][softmax::kLdsWords];
  __shared__ float s_fin[4][64 * 3];                // per position: g, then (m, G, pos coefficient)
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = lane / LPR, sl = lane % LPR;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  float* const zl = s_z[wave];
  int32_t* const idl = s_id[wave];
  float* const fin = s_fin[wave];
  const int d = a.d, K = a.k, C = a.chunk;
  const int stride = softmax::lds_stride(K);
  const uint32_t magic = a.magic;
  const float inv_tau = a.inv_tau;
  float lsum = 0.f;   // per-lane loss sum, on each slot's first lane
  if (u < a.n_users) {
    const float ge = *a.cscale * a.inv_e;
    const int64_t beg = a.rowptr[u], end = a.rowptr[u + 1];
    typename V::T uv[VPL], acc[VPL];
#pragma unroll
    for (int q = 0; q < VPL; ++q) {
      const int cc = (q * LPR + sl) * W;
      uv[q] = cc < d ? S::widen(S::load(Ux + u * d + cc)) : V::zero();
      acc[q] = V::zero();
    }
    // flat negative r of a chunk (r < C * K <= kLdsWords) -> its word: [r / K][1 + r % K]
    auto word_of = [&](int r) -> int {
      const int pos = (int)(((uint32_t)r * magic) >> 20);
      return pos * stride + 1 + (r - pos * K);
    };
    for (int64_t base = beg; base < end; base += C) {
      const int n = (int)min<int64_t>(C, end - base);
      const int R = n * K;
      const int64_t first = base * K;
      // ---- the chunk's ids, offsets and scales into LDS, each checked once
      if (lane < n) {
        const int pid = a.col[base + lane];
        float g = ge;
        if (a.edge_w) g *= a.edge_w[base + lane];
        idl[lane * stride] = pid;
        zl[lane * stride] = a.post_bias ? a.post_bias[pid] : 0.f;
        fin[lane * 3] = g;
      }
      for (int r = lane; r < R; r += 64) {
        const int64_t nn = a.neg32 ? (int64_t)a.neg32[first + r] : a.neg[first + r];
        const int w = word_of(r);
        if (nn < 0 || nn >= a.n_posts) {
          if (a.err) atomicAdd(a.err, 1);
          idl[w] = -1;
          zl[w] = __builtin_inff();   // the logit becomes -inf: softmax::masked()
        } else {
          idl[w] = (int32_t)nn;
          zl[w] = a.post_bias ? a.post_bias[nn] : 0.f;
        }
      }
      // the wave's own LDS writes, read back by other lanes: ordered within the wave
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // ---- the chunk's rows: edge step es holds edges es * NS + slot, row j of each
      const int nsteps = (n + NS - 1) / NS;
      const int T = nsteps * (K + 1);
      softmax::State st = softmax::open(0.f);
      typename V::T ae[VPL], p0v[VPL];
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        ae[q] = V::zero();
        p0v[q] = V::zero();
      }
      auto load_row = [&](int es, int j, Raw (&x)[VPL]) {
        const int e = es * NS + slot;
        const int ee = e < n ? e : 0;             // (past the chunk: position 0's ids)
        const int id = idl[ee * stride + j];
        const int64_t r0 = id > 0 ? id : 0;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int cc = (q * LPR + sl) * W;
          const int ccl = cc < d ? cc : 0;
          x[q] = S::load(Px + r0 * d + ccl);
        }
      };
      auto score_row = [&](int es, int j, const Raw (&x)[VPL]) {
        if (es >= nsteps) return;                 // (wave-uniform: the ping-pong's overhang)
        const int e = es * NS + slot;
        const bool live = e < n;
        const int ee = live ? e : 0;
        const int w = ee * stride + j;
        typename V::T v[VPL];
#pragma unroll
        for (int q = 0; q < VPL; ++q) v[q] = S::widen(x[q]);
        const float s = slot_dot<LPR, VPL, W>(uv, v);
        // a slot past the chunk carries a finite dummy edge; its scale below is 0
        const float z = live ? s * inv_tau - zl[w] : 0.f;
        if (j == 0) {
          st = softmax::open(z);
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            p0v[q] = v[q];
            ae[q] = V::zero();
          }
        } else {
          const softmax::Step t = softmax::update(st, z);
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            V::scale(ae[q], t.rescale);
            V::fma(ae[q], t.w, v[q]);
          }
        }
        if (sl == 0 && live) zl[w] = z;           // parked for the coefficients
        if (j == K) {
          const float g = live ? fin[ee * 3] : 0.f;
          const softmax::Closed c = softmax::close(st, g, inv_tau);
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            V::fma(acc[q], c.G, ae[q]);
            V::fma(acc[q], c.pos, p0v[q]);
          }
          if (sl == 0 && live) {
            lsum += g * c.loss;
            fin[e * 3] = st.m;
            fin[e * 3 + 1] = c.G;
            fin[e * 3 + 2] = c.pos;
          }
        }
      };
      // cursors of the loads (one step ahead) and of the scoring over the flat row sequence
      int les = 0, lj = 0, ses = 0, sj = 0;
      auto ld = [&](Raw (&x)[VPL]) {
        load_row(les, lj, x);
        if (++lj > K) { lj = 0; ++les; }
      };
      auto go = [&](const Raw (&x)[VPL]) {
        score_row(ses, sj, x);
        if (++sj > K) { sj = 0; ++ses; }
      };
      Raw a0[VPL], a1[VPL], b0[VPL], b1[VPL];
      ld(a0);
      ld(a1);
      for (int t = 0; t < T; t += 4) {
        ld(b0);
        ld(b1);
        go(a0);
        go(a1);
        if (t + 2 >= T) break;
        ld(a0);
        ld(a1);
        go(b0);
        go(b1);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // ---- the parked logits under each edge's final (m, G): the pairs' coefficients
      for (int r = lane; r < R; r += 64) {
        const int pos = (int)(((uint32_t)r * magic) >> 20);
        const float z = zl[pos * stride + 1 + (r - pos * K)];
        a.coef_neg[first + r] = softmax::neg_coef(z, fin[pos * 3], fin[pos * 3 + 1]);
      }
      if (lane < n) {
        const int64_t p = base + lane;
        a.coef_pos[a.slot_of ? (int64_t)a.slot_of[p] : p] = fin[lane * 3 + 2];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1)
#pragma unroll
      for (int q = 0; q < VPL; ++q) V::add(acc[q], V::shfl_xor(acc[q], m));
    if (lane < LPR) {
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        const int cc = (q * LPR + sl) * W;
        if (cc < d) V::store(a.dU + u * d + cc, acc[q]);
      }
    }
  }
  // deterministic block partials, as k_edge_score: wave tree, then waves in order
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) lsum += __shfl_xor(lsum, m, 64);
  if (lane == 0) red[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) a.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Deterministic two-level reduction of the block partials (scoring.hip's chain with one sum): 64
// blocks each sum a contiguous range in double, then one thread adds the 64 in order.  The
// partials carry their scales already, so the loss is their plain sum.
constexpr int kSmRedBlocks = 64;

__global__ void __launch_bounds__(256) k_softmax_loss_partial(const float* part, int64_t n_part,
                                                              double* red) {
  __shared__ double sp[256];
  const int64_t per = cdiv(n_part, kSmRedBlocks);
  const int64_t b0 = blockIdx.x * per, b1 = min<int64_t>(b0 + per, n_part);
  double p = 0.0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) p += part[i];
  sp[threadIdx.x] = p;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sp[threadIdx.x] += sp[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) red[blockIdx.x] = sp[0];
}

__global__ void k_softmax_loss_final(const double* red, float* loss) {
  if (threadIdx.x != 0) return;
  double p = 0.0;
  for (int i = 0; i < kSmRedBlocks; ++i) p += red[i];
  *loss = (float)p;
}

template <int LPR, int VPL, int W, typename XT = float>
static int launch_softmax(const SoftmaxArgs& a, int64_t nblocks, hipStream_t stream) {
  hipLaunchKernelGGL((k_edge_softmax<LPR, VPL, W, XT>), dim3((unsigned)nblocks), dim3(256), 0,
                     stream, a);
  return check_launch("k_edge_softmax");
}

// floats of `part`: one per block of 4 user-waves, then room for 64 doubles, 16-B aligned
static int64_t softmax_parts(int64_t n_users) {
  return (int64_t)align_up((size_t)cdiv(n_users, 4), 4) + 2 * kSmRedBlocks;
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int32_t hgnn_softmax_chunk(int32_t n_neg) { return softmax::chunk(n_neg); }

int64_t hgnn_softmax_parts(int64_t n_users) { return softmax_parts(n_users < 0 ? 0 : n_users); }

int hgnn_edge_softmax_fwd(int32_t rows, const void* U, const void* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                          int32_t n_neg, int64_t n_edges, const float* cscale,
                          const float* post_bias, float temperature, const int32_t* slot_of,
                          float* dU, float* coef_pos, float* coef_neg, float* part, float* loss,
                          int32_t* err, hgnn_stream_t stream_) {
  const char* who = "edge_softmax_fwd";
  hipStream_t stream = as_stream(stream_);
  // every rule before any launch
  if (rows != HGNN_ROWS_F32 && rows != HGNN_ROWS_BF16)
    return fail(HGNN_E_ARG, "%s: rows=%d (fp32 or bf16 rows)", who, rows);
  if (d < 1 || n_users < 0 || n_posts < 0 || n_edges < 0)
    return fail(HGNN_E_ARG, "%s: bad sizes (d=%d, n_users=%lld, n_posts=%lld, n_edges=%lld)", who,
                d, (long long)n_users, (long long)n_posts, (long long)n_edges);
  if (n_neg < 1 || n_neg > softmax::kMaxNeg)
    return fail(HGNN_E_ARG, "%s: n_neg=%d (1 <= n_neg <= %d)", who, n_neg, softmax::kMaxNeg);
  if (!(temperature > 0.f) || !isfinite(temperature))
    return fail(HGNN_E_ARG, "%s: temperature=%g (finite and > 0)", who, (double)temperature);
  if (n_edges * (int64_t)n_neg >= (int64_t(1) << 31) - 1)
    return fail(HGNN_E_ARG, "%s: %lld edges x n_neg=%d reach the negatives sort's limit of "
                            "2^31 - 1 pairs", who, (long long)n_edges, n_neg);
  if (rows == HGNN_ROWS_BF16 && (d % 8 != 0 || d > 512))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (bf16 rows need d %% 8 == 0 and d <= 512)", who, d);
  if (rows == HGNN_ROWS_F32 && d > 512)
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (fp32 rows need d <= 512)", who, d);
  if (!cscale || !loss || !part || (n_users > 0 && (!U || !rowptr_u || !dU)))
    return fail(HGNN_E_ARG, "%s: null pointer", who);
  if (n_edges > 0 && (!P || !col_u || !coef_pos || !coef_neg))
    return fail(HGNN_E_ARG, "%s: null pointer", who);
  const int given = (neg_i64 != nullptr) + (neg_i32 != nullptr);
  if (given > 1 || (n_edges > 0 && given != 1))
    return fail(HGNN_E_ARG, "%s: the negatives come in exactly one form (int64 or int32)", who);
  if (err) (void)hipMemsetAsync(err, 0, sizeof(int32_t), stream);   // (null: not counted)
  SoftmaxArgs a{};
  a.U = U; a.P = P; a.rowptr = rowptr_u; a.col = col_u; a.neg = neg_i64; a.neg32 = neg_i32;
  a.edge_w = edge_w; a.post_bias = post_bias; a.slot_of = slot_of; a.cscale = cscale;
  a.dU = dU; a.coef_pos = coef_pos; a.coef_neg = coef_neg; a.part = part; a.err = err;
  a.n_users = n_users; a.n_posts = n_posts;
  a.inv_e = n_edges > 0 ? 1.f / (float)n_edges : 0.f;
  a.inv_tau = 1.f / temperature;
  a.d = d; a.k = n_neg; a.chunk = softmax::chunk(n_neg);
  a.magic = (uint32_t)(((1u << 20) + n_neg - 1) / n_neg);
  const int64_t nb = cdiv(n_users, 4);   // blocks of 4 user-waves
  if (nb > 0) {
    int rc;
    if (rows == HGNN_ROWS_BF16) {   // the widths of edge_score_fwd
      using B = uint16_t;
      if (d <= 64) rc = launch_softmax<8, 1, 8, B>(a, nb, stream);
      else if (d <= 128) rc = launch_softmax<16, 1, 8, B>(a, nb, stream);
      else if (d <= 256) rc = launch_softmax<32, 1, 8, B>(a, nb, stream);
      else rc = launch_softmax<64, 1, 8, B>(a, nb, stream);
    }
    else if (d % 4 == 0 && d <= 64) rc = launch_softmax<16, 1, 4>(a, nb, stream);
    else if (d % 4 == 0 && d <= 128) rc = launch_softmax<32, 1, 4>(a, nb, stream);
    else if (d % 4 == 0 && d <= 256) rc = launch_softmax<64, 1, 4>(a, nb, stream);
    else if (d <= 64) rc = launch_softmax<64, 1, 1>(a, nb, stream);
    else rc = launch_softmax<64, 8, 1>(a, nb, stream);
    if (rc) return rc;
  }
  // the reduction scratch lives after the block partials
  double* red = reinterpret_cast<double*>(part + align_up((size_t)nb, 4));
  hipLaunchKernelGGL(k_softmax_loss_partial, dim3(kSmRedBlocks), dim3(256), 0, stream, part, nb,
                     red);
  if (int rc = check_launch("k_softmax_loss_partial")) return rc;
  hipLaunchKernelGGL(k_softmax_loss_final, dim3(1), dim3(64), 0, stream, red, loss);
  return check_launch("k_softmax_loss_final");
}

}  // extern "C"
