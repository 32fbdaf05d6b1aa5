// Hard (model-scored) negatives for the link loss: of M candidate posts per positive edge, the k
// the current tables score highest (hgnn_hard_negatives; the contract per position is in
// include/hgnn.h, the selection rounds in hardneg_select.h).
//
// The scoring pass's shape (scoring.hip, k_edge_score_k): one wave per user keeps U[u] in
// registers and streams post rows through two register sets in ping-pong, LPR lanes per row.  A
// wave takes its user's positions in chunks of C (hard_neg_chunk(M)).  A chunk's C * M candidates
// are contiguous in the [E, M] array, so they are walked as one flat list: groups of 64 ids, one
// coalesced load per group (lane = row of the group; drawn pools compute uniform_draw there), the
// id reaching the lanes that load its row by a shuffle; a step takes 2 * NS rows (two per slot,
// the bytes in flight of the scoring pass's two-row step) and the pipeline runs across group
// boundaries: a group's ids are loaded a whole group ahead.  The slot's first lane parks each
// score, and the lane that loaded an id parks it (-1 if out of range, counted into err there, once)
// in two per-wave LDS arrays at [position][column] with an odd stride.  After the chunk's rows,
// lane = position runs the k selection rounds over its own M scores and ids and writes its k ids.
// No dU, no exp, no loss: ids out, and the two counters are the only atomics.
//
// LDS: 2 arrays x 4 waves x kLdsWords x 4 B = 20 KiB per block, so 8 blocks = 32 waves fit a
// CU's 160 KiB and LDS allows what the wave limit does.  C = min(64, kLdsWords / (M | 1)).
#include "hgnn_common.h"
#include "hardneg_select.h"

namespace hgnn {

constexpr int kHnLdsWords = 640;   // per wave and array: 64 positions at M <= 9, 9 at M = 64

static int32_t hard_neg_chunk(int32_t m) {
  if (m < 1 || m > hardneg::kMaxCand) return 0;
  const int c = kHnLdsWords / hardneg::lds_stride(m);
  return c < 64 ? c : 64;
}

struct HardNegArgs {
  const void* U;               // fp32 rows, or bf16 rows in the XT = uint16_t instantiation
  const void* P;
  const int32_t* rowptr;       // user-grouped CSR of the positive edges
  const int32_t* col;          // positive post per position
  const int32_t* cand;         // [E, m] candidates in the user-grouped order ...
  const uint64_t* seed;        // ... or drawn here: uniform_draw(*seed, p * m + j, n_posts)
  int32_t* out;                // [E, k]
  unsigned long long* short_count;
  int32_t* err;
  int64_t n_users;
  int64_t n_posts;
  int32_t d, m, k, chunk;
  uint32_t magic;              // ceil(2^20 / m): r / m = (r * magic) >> 20 for r < 4096
};

// The candidates' rows are read with plain loads whatever the pool and the table size: nt loads
// (the scoring pass's policy for its uniform negatives over a table past the Infinity Cache) were
// measured on a uniform pool at cfg4, fp32 rows, and lost, 125.4 ms against 109.6 at M = 8 and
// 65.8 against 55.0 at M = 4 (profiles/hard_neg_nt_ab.jsonl): here no positives' rows compete for
// the cache, and the candidates' own re-reads are worth keeping.
template <int LPR, int VPL, int W, typename XT>
__global__ void __launch_bounds__(256) k_hard_negatives(const HardNegArgs a) {
  using V = Vec<W>;
  using S = RowSrc<XT, W>;
  using Raw = typename S::Raw;
  const XT* const Ux = static_cast<const XT*>(a.U);
  const XT* const Px = static_cast<const XT*>(a.P);
  constexpr int NS = 64 / LPR;      // slots: rows per half step
  constexpr int RS = 2 * NS;        // rows per step (divides 64: a step never straddles a group)
  static_assert(64 % (2 * RS) == 0, "a group of 64 rows is an even number of steps");
  __shared__ float s_sc[4][kHnLdsWords];
  __shared__ int32_t s_id[4][kHnLdsWords];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = lane / LPR, sl = lane % LPR;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= a.n_users) return;       // (no block-wide barrier in this kernel)
  float* const sc = s_sc[wave];
  int32_t* const idl = s_id[wave];
  const int d = a.d, M = a.m, K = a.k, C = a.chunk;
  const int stride = hardneg::lds_stride(M);
  const uint32_t np = (uint32_t)a.n_posts, magic = a.magic;
  const bool seed_p = a.seed != nullptr;
  const uint64_t seed = seed_p ? *a.seed : 0;
  const int64_t beg = a.rowptr[u], end = a.rowptr[u + 1];
  typename V::T uv[VPL];
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    const int cc = (q * LPR + sl) * W;
    uv[q] = cc < d ? S::widen(S::load(Ux + u * d + cc)) : V::zero();
  }
  // row r of a chunk (r < C * M <= kHnLdsWords) -> its word in the LDS arrays
  auto word_of = [&](int r) -> int {
    const int pos = (int)(((uint32_t)r * magic) >> 20);
    return pos * stride + (r - pos * M);
  };
  int n_short = 0;
  for (int64_t base = beg; base < end; base += C) {
    const int n = (int)min<int64_t>(C, end - base);
    const int R = n * M;            // the chunk's rows
    const int64_t first = base * M;
    int pid = 0;
    if (lane < n) pid = a.col[base + lane];
    // the id of row g * 64 + lane as loaded (or drawn); 0 past the chunk.  Unchecked: the row
    // loads clamp it, park() checks it once its group is the current one
    auto load_raw = [&](int g) -> int {
      const int r = g * 64 + lane;
      if (r >= R) return 0;
      return seed_p ? uniform_draw(seed, first + r, np) : a.cand[first + r];
    };
    auto park = [&](int g, int raw) {
      const int r = g * 64 + lane;
      if (r < R) {
        int id = raw;
        if ((uint32_t)raw >= np) {
          if (a.err) atomicAdd(a.err, 1);
          id = -1;
        }
        idl[word_of(r)] = id;
      }
    };
    // The steps of k_edge_score (its comment on the unconditional loads holds here): rows past
    // the chunk and out-of-range ids read post 0, columns past d read column 0; none of them
    // reaches a result (their scores are not parked, uv is 0 past d).
    Raw a0[VPL], a1[VPL], b0[VPL], b1[VPL];
    auto load_step = [&](int raw, int j, Raw (&x0)[VPL], Raw (&x1)[VPL]) {
      const int e = j + slot;
      const uint32_t i0 = (uint32_t)__shfl(raw, e & 63, 64);
      const uint32_t i1 = (uint32_t)__shfl(raw, (e + NS) & 63, 64);
      const int64_t r0 = i0 < np ? i0 : 0, r1 = i1 < np ? i1 : 0;
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        const int cc = (q * LPR + sl) * W;
        const int ccl = cc < d ? cc : 0;
        x0[q] = S::load(Px + r0 * d + ccl);
        x1[q] = S::load(Px + r1 * d + ccl);
      }
    };
    auto score_step = [&](int g, int j, const Raw (&x0)[VPL], const Raw (&x1)[VPL]) {
      const int r = g * 64 + j + slot;
      typename V::T v0[VPL], v1[VPL];
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        v0[q] = S::widen(x0[q]);
        v1[q] = S::widen(x1[q]);
      }
      const float s0 = slot_dot<LPR, VPL, W>(uv, v0);
      const float s1 = slot_dot<LPR, VPL, W>(uv, v1);
      if (sl == 0) {
        if (r < R) sc[word_of(r)] = s0;
        if (r + NS < R) sc[word_of(r + NS)] = s1;
      }
    };
    int cur = load_raw(0);
    load_step(cur, 0, a0, a1);
    for (int g = 0; g * 64 < R; ++g) {
      const int nxt = load_raw(g + 1);
      park(g, cur);
      const int rg = min(64, R - g * 64);
      for (int j = 0; j < rg; j += 2 * RS) {
        load_step(cur, j + RS, b0, b1);
        score_step(g, j, a0, a1);
        if (j + RS >= rg) break;
        // (the group's last step prefetches the next group's first rows)
        load_step(j + 2 * RS < 64 ? cur : nxt, (j + 2 * RS) & 63, a0, a1);
        score_step(g, j + RS, b0, b1);
      }
      cur = nxt;
    }
    // the wave's own LDS writes, read back lane = position: ordered within the wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < n)
      n_short += hardneg::select_k(sc + lane * stride, idl + lane * stride, M, K, pid,
                                   a.n_posts, a.out + (base + lane) * K);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (a.short_count) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n_short += __shfl_xor(n_short, m, 64);
    if (lane == 0 && n_short) atomicAdd(a.short_count, (unsigned long long)n_short);
  }
}

template <int LPR, int VPL, int W, typename XT = float>
static int launch_hard_neg(const HardNegArgs& a, int64_t nblocks, hipStream_t stream) {
  hipLaunchKernelGGL((k_hard_negatives<LPR, VPL, W, XT>), dim3((unsigned)nblocks), dim3(256), 0,
                     stream, a);
  return check_launch("k_hard_negatives");
}

// every rule before any launch; `who` words them
static int hard_negatives(const char* who, bool bf16, const void* U, const void* P, int32_t d,
                          int64_t n_users, int64_t n_posts, const int32_t* rowptr_u,
                          const int32_t* col_u, const int32_t* cand32, const uint64_t* cand_seed,
                          int32_t n_cand, int32_t n_neg, int32_t* out, int64_t* short_count,
                          int32_t* err, hgnn_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  if (d < 1 || n_users < 0 || n_posts < 1 || n_posts >= (int64_t(1) << 31) - 1)
    return fail(HGNN_E_ARG, "%s: bad sizes (d=%d, n_users=%lld, n_posts=%lld)", who, d,
                (long long)n_users, (long long)n_posts);
  if (n_neg < 1 || n_cand < n_neg || n_cand > hardneg::kMaxCand)
    return fail(HGNN_E_ARG, "%s: n_neg=%d, n_cand=%d (1 <= n_neg <= n_cand <= %d)", who, n_neg,
                n_cand, hardneg::kMaxCand);
  if (bf16 && (d % 8 != 0 || d > 512))
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (bf16 rows need d %% 8 == 0 and d <= 512)", who, d);
  if (!bf16 && d > 512)
    return fail(HGNN_E_UNSUPPORTED, "%s: d=%d (fp32 rows need d <= 512)", who, d);
  if (!U || !P || !rowptr_u || !col_u || !out) return fail(HGNN_E_ARG, "%s: null pointer", who);
  if ((cand32 != nullptr) == (cand_seed != nullptr))
    return fail(HGNN_E_ARG, "%s: the candidates come in exactly one form (cand32 or cand_seed)",
                who);
  if (err) (void)hipMemsetAsync(err, 0, sizeof(int32_t), stream);   // (null: not counted)
  HardNegArgs a{};
  a.U = U; a.P = P; a.rowptr = rowptr_u; a.col = col_u; a.cand = cand32; a.seed = cand_seed;
  a.out = out; a.short_count = reinterpret_cast<unsigned long long*>(short_count); a.err = err;
  a.n_users = n_users; a.n_posts = n_posts; a.d = d; a.m = n_cand; a.k = n_neg;
  a.chunk = hard_neg_chunk(n_cand);
  a.magic = (uint32_t)(((1u << 20) + n_cand - 1) / n_cand);
  const int64_t nb = cdiv(n_users, 4);   // blocks of 4 user-waves
  if (nb == 0) return HGNN_OK;
  if (bf16) {   // the widths of edge_score_fwd
    using B = uint16_t;
    if (d <= 64) return launch_hard_neg<8, 1, 8, B>(a, nb, stream);
    if (d <= 128) return launch_hard_neg<16, 1, 8, B>(a, nb, stream);
    if (d <= 256) return launch_hard_neg<32, 1, 8, B>(a, nb, stream);
    return launch_hard_neg<64, 1, 8, B>(a, nb, stream);
  }
  if (d % 4 == 0 && d <= 64) return launch_hard_neg<16, 1, 4>(a, nb, stream);
  if (d % 4 == 0 && d <= 128) return launch_hard_neg<32, 1, 4>(a, nb, stream);
  if (d % 4 == 0 && d <= 256) return launch_hard_neg<64, 1, 4>(a, nb, stream);
  if (d <= 64) return launch_hard_neg<64, 1, 1>(a, nb, stream);
  return launch_hard_neg<64, 8, 1>(a, nb, stream);
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int32_t hgnn_hard_neg_chunk(int32_t n_cand) { return hard_neg_chunk(n_cand); }

int32_t hgnn_hard_neg_lds_words(void) { return kHnLdsWords; }

int hgnn_hard_negatives(const float* U, const float* P, int32_t d, int64_t n_users,
                        int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                        const int32_t* cand32, const uint64_t* cand_seed, int32_t n_cand,
                        int32_t n_neg, int32_t* out, int64_t* short_count, int32_t* err,
                        hgnn_stream_t stream) {
  return hard_negatives("hard_negatives", false, U, P, d, n_users, n_posts, rowptr_u, col_u,
                        cand32, cand_seed, n_cand, n_neg, out, short_count, err, stream);
}

int hgnn_hard_negatives_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const int32_t* cand32, const uint64_t* cand_seed, int32_t n_cand,
                             int32_t n_neg, int32_t* out, int64_t* short_count, int32_t* err,
                             hgnn_stream_t stream) {
  return hard_negatives("hard_negatives_bf16", true, U, P, d, n_users, n_posts, rowptr_u, col_u,
                        cand32, cand_seed, n_cand, n_neg, out, short_count, err, stream);
}

}  // extern "C"
