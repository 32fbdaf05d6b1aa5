// Popularity-weighted negatives: the table of a discrete distribution over the posts, built on
// the device once per distribution, and the per-step draws from it.
//
//   q[n_posts]        integer weights, each in [0, 2^32), sum T in [1, 2^63)
//   cdf[n_posts + 1]  exclusive cumulative sums of q (int64, exact in any summation order)
//   draw c            x = splitmix64(seed + c * golden)  (uniform_draw's word before its shift)
//                     r = (x * T) >> 64                  (high half of the 64 x 64-bit product)
//                     the unique post j with cdf[j] <= r < cdf[j + 1]
//
// A post of weight 0 has cdf[j] == cdf[j + 1] and is never drawn.  The search is a binary search
// between two entries of a guide table: guide[b] = the post that holds the value b << shift, so a
// draw with r >> shift == b lies in [guide[b], guide[b + 1]].  With as many buckets as posts a
// bucket holds about one post of average weight, and the search is a step or two on lines the
// bucket's neighbours have just read.  One lane per draw: the kernels are latency-bound on a
// table that the caches hold (1M posts: 8 MB of cdf and 4 MB of guide).
//
// Rejection (hgnn_weighted_avoid_i32): draw i = p * k + j of user-grouped position p tries the
// counters i, i + n, i + 2 n, ... (n = E * k draws) and keeps the first post that the position's
// user has not seen (a binary search in the user's ascending seen list); if every try is seen it
// keeps the last and counts it.  Plain C++, vector loads and stores, one atomicAdd per wave.
#include "hgnn_common.h"

namespace hgnn {

// ------------------------------------------------------------------------------------------
// Exclusive scan of int64 (exclusive_scan_i32's three phases on 64-bit sums).
// ------------------------------------------------------------------------------------------
constexpr int kScan64Threads = 256;
constexpr int kScan64Items = 8;                              // per thread
constexpr int kScan64Tile = kScan64Threads * kScan64Items;   // 2048

__device__ __forceinline__ int64_t wave_incl_scan64(int64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// block-wide exclusive scan of one value per thread; the block total in *total
__device__ __forceinline__ int64_t block_excl_scan64(int64_t v, int64_t* lds, int64_t* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t inc = wave_incl_scan64(v);
  if (lane == 63) lds[wid] = inc;
  __syncthreads();
  int64_t wpre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kScan64Threads / 64; ++w) {
    const int64_t s = lds[w];
    wpre += (w < wid) ? s : 0;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return wpre + inc - v;
}

__global__ void __launch_bounds__(kScan64Threads) k_tile_sums64(const int64_t* in, int64_t n,
                                                                int64_t* sums) {
  __shared__ int64_t lds[kScan64Threads / 64];
  const int64_t base = (int64_t)blockIdx.x * kScan64Tile;
  int64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScan64Items; ++i) {
    const int64_t idx = base + (int64_t)i * kScan64Threads + threadIdx.x;
    s += idx < n ? in[idx] : 0;
  }
  int64_t tot;
  block_excl_scan64(s, lds, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// out[i] = offs[tile] + exclusive prefix of in within the tile; the last tile writes out[n]
__global__ void __launch_bounds__(kScan64Threads) k_tile_scan64(const int64_t* in, int64_t n,
                                                                const int64_t* offs,
                                                                int64_t* out) {
  __shared__ int64_t lds[kScan64Threads / 64];
  const int64_t base = (int64_t)blockIdx.x * kScan64Tile + (int64_t)threadIdx.x * kScan64Items;
  int64_t v[kScan64Items];
  int64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScan64Items; ++i) {
    const int64_t idx = base + i;
    v[i] = idx < n ? in[idx] : 0;
    s += v[i];
  }
  int64_t tot;
  int64_t pre = block_excl_scan64(s, lds, &tot) + (offs ? offs[blockIdx.x] : 0);
#pragma unroll
  for (int i = 0; i < kScan64Items; ++i) {
    const int64_t idx = base + i;
    if (idx < n) out[idx] = pre;
    pre += v[i];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kScan64Threads - 1) out[n] = pre;
}

static size_t scan64_ws_bytes(int64_t n) {
  size_t b = 0;
  while (n > kScan64Tile) {
    const int64_t t = cdiv(n, kScan64Tile);
    b += align_up((size_t)(t + 1) * 8, 256);
    n = t;
  }
  return b + 256;
}

// n >= 1; in and out may be the same array only where one tile holds it (the nested call)
static int exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, void* ws,
                              size_t ws_bytes, hipStream_t stream) {
  const int64_t tiles = cdiv(n, kScan64Tile);
  if (tiles == 1) {
    hipLaunchKernelGGL(k_tile_scan64, dim3(1), dim3(kScan64Threads), 0, stream, in, n,
                       (const int64_t*)nullptr, out);
    return check_launch("k_tile_scan64");
  }
  Workspace w(ws, ws_bytes);
  int64_t* sums = w.take<int64_t>(tiles + 1);
  if (!sums) return fail(HGNN_E_WS, "cdf scan: workspace too small");
  const size_t off = align_up(w.used, 256);
  const size_t rest = w.cap > off ? w.cap - off : 0;
  hipLaunchKernelGGL(k_tile_sums64, dim3((unsigned)tiles), dim3(kScan64Threads), 0, stream, in, n,
                     sums);
  if (int rc = check_launch("k_tile_sums64")) return rc;
  if (int rc = exclusive_scan_i64(sums, sums, tiles, w.base + off, rest, stream)) return rc;
  hipLaunchKernelGGL(k_tile_scan64, dim3((unsigned)tiles), dim3(kScan64Threads), 0, stream, in, n,
                     (const int64_t*)sums, out);
  return check_launch("k_tile_scan64");
}

// ------------------------------------------------------------------------------------------
// The search and the draws.
// ------------------------------------------------------------------------------------------
struct WeightedTable {
  const int64_t* cdf;     // [n_posts + 1]; null: the uniform distribution over n_posts
  const int32_t* guide;   // [n_guide + 1]
  uint64_t T;
  int32_t n_posts;
  int32_t shift;          // bucket of r = r >> shift, below n_guide
  int32_t n_guide;
};

__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t c) {
  uint64_t x = seed + c * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the post j in [lo, hi] with cdf[j] <= r < cdf[j + 1], given that it lies in that range:
// the first j whose cdf[j + 1] exceeds r
__device__ __forceinline__ int32_t cdf_search(const int64_t* cdf, int64_t r, int32_t lo,
                                              int32_t hi) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cdf[mid + 1] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int32_t weighted_draw(const WeightedTable& t, uint64_t seed,
                                                 uint64_t c) {
  const uint64_t x = splitmix64_at(seed, c);
  if (!t.cdf) return (int32_t)(((x >> 32) * (uint64_t)(uint32_t)t.n_posts) >> 32);
  const int64_t r = (int64_t)__umul64hi(x, t.T);          // < T < 2^63
  int64_t b = r >> t.shift;
  if (b >= t.n_guide) b = t.n_guide - 1;                  // (never: (T - 1) >> shift < n_guide)
  int32_t lo = t.guide[b], hi = t.guide[b + 1];
  lo = min(max(lo, 0), t.n_posts - 1);                    // a guide entry is an index into cdf
  hi = min(max(hi, lo), t.n_posts - 1);
  return cdf_search(t.cdf, r, lo, hi);
}

// guide[b] for b in [0, n_guide]: the post holding b << shift, or the last post where that value
// is T or more (an upper bound of every draw)
__global__ void __launch_bounds__(256) k_guide_build(const int64_t* cdf, int32_t n_posts,
                                                     int64_t T, int32_t shift, int32_t n_guide,
                                                     int32_t* guide) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > n_guide) return;
  const uint64_t v = (uint64_t)b << shift;      // (at most 2^63: unsigned)
  guide[b] = v >= (uint64_t)T ? n_posts - 1 : cdf_search(cdf, (int64_t)v, 0, n_posts - 1);
}

__global__ void __launch_bounds__(256) k_weighted_i32(const uint64_t* seed, int64_t n,
                                                      const WeightedTable t, int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = weighted_draw(t, *seed, (uint64_t)i);
}

// whether `post` is in the ascending list col[beg, end)
__device__ __forceinline__ bool seen_has(const int32_t* col, int32_t beg, int32_t end,
                                         int32_t post) {
  while (beg < end) {
    const int32_t mid = beg + ((end - beg) >> 1);
    const int32_t v = col[mid];
    if (v == post) return true;
    if (v < post) beg = mid + 1; else end = mid;
  }
  return false;
}

__global__ void __launch_bounds__(256) k_weighted_avoid_i32(
    const uint64_t* seed, int64_t n, int32_t k, const WeightedTable t, const int32_t* user_of_pos,
    int64_t n_users, const int32_t* seen_rowptr, const int32_t* seen_col, int32_t tries,
    int32_t* out, unsigned long long* kept_seen) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool kept = false;
  if (i < n) {
    const uint64_t s = *seed;
    const int32_t u = user_of_pos[i / k];
    int32_t beg = 0, end = 0;
    if (u >= 0 && u < n_users) {               // (a user outside the seen index has seen nothing)
      beg = seen_rowptr[u];
      end = seen_rowptr[u + 1];
    }
    int32_t post = 0;
    bool seen = true;
    for (int32_t a = 0; a < tries && seen; ++a) {
      post = weighted_draw(t, s, (uint64_t)i + (uint64_t)a * (uint64_t)n);
      seen = seen_has(seen_col, beg, end, post);
    }
    out[i] = post;
    kept = seen;
  }
  const unsigned long long m = __ballot(kept);
  if (kept_seen && m && (threadIdx.x & 63) == 0)
    atomicAdd(kept_seen, (unsigned long long)__popcll(m));
}

static int guide_rule(const char* who, const int64_t* cdf, int64_t n_posts, int64_t T,
                      const int32_t* guide, int32_t shift, int32_t n_guide) {
  if (n_posts < 1 || n_posts >= (int64_t(1) << 31))
    return fail(HGNN_E_ARG, "%s: n_posts=%lld out of range", who, (long long)n_posts);
  if (!cdf) return HGNN_OK;
  if (T < 1) return fail(HGNN_E_ARG, "%s: T=%lld (the weights' sum must be at least 1)", who,
                         (long long)T);
  if (!guide) return fail(HGNN_E_ARG, "%s: null guide", who);
  if (shift < 0 || shift > 62 || n_guide < 1 || ((T - 1) >> shift) >= n_guide)
    return fail(HGNN_E_ARG, "%s: guide of %d buckets at shift %d does not cover T=%lld", who,
                n_guide, shift, (long long)T);
  return HGNN_OK;
}

static WeightedTable table_of(const int64_t* cdf, int64_t n_posts, int64_t T,
                              const int32_t* guide, int32_t shift, int32_t n_guide) {
  WeightedTable t{};
  t.cdf = cdf; t.guide = guide; t.T = (uint64_t)T; t.n_posts = (int32_t)n_posts;
  t.shift = shift; t.n_guide = n_guide;
  return t;
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

size_t hgnn_weighted_cdf_ws_bytes(int64_t n_posts) {
  return scan64_ws_bytes(n_posts < 1 ? 1 : n_posts) + 2048;
}

int hgnn_weighted_cdf_build(const int64_t* q, int64_t n_posts, int64_t* cdf, void* ws,
                            size_t ws_bytes, hgnn_stream_t stream) {
  if (n_posts < 1 || n_posts >= (int64_t(1) << 31))
    return fail(HGNN_E_ARG, "weighted_cdf_build: n_posts=%lld out of range", (long long)n_posts);
  if (!q || !cdf) return fail(HGNN_E_ARG, "weighted_cdf_build: null pointer");
  if (n_posts > kScan64Tile && (!ws || ws_bytes < scan64_ws_bytes(n_posts)))
    return fail(HGNN_E_WS, "weighted_cdf_build: workspace too small");
  return exclusive_scan_i64(q, cdf, n_posts, ws, ws_bytes, as_stream(stream));
}

int hgnn_weighted_guide_build(const int64_t* cdf, int64_t n_posts, int64_t T, int32_t shift,
                              int32_t n_guide, int32_t* guide, hgnn_stream_t stream) {
  if (!cdf) return fail(HGNN_E_ARG, "weighted_guide_build: null cdf");
  if (int rc = guide_rule("weighted_guide_build", cdf, n_posts, T, guide, shift, n_guide))
    return rc;
  hipLaunchKernelGGL(k_guide_build, dim3((unsigned)cdiv((int64_t)n_guide + 1, 256)), dim3(256), 0,
                     as_stream(stream), cdf, (int32_t)n_posts, T, shift, n_guide, guide);
  return check_launch("k_guide_build");
}

int hgnn_weighted_i32(const uint64_t* d_seed, int64_t n, const int64_t* cdf, int64_t n_posts,
                      int64_t T, const int32_t* guide, int32_t shift, int32_t n_guide,
                      int32_t* out, hgnn_stream_t stream) {
  if (n < 0) return fail(HGNN_E_ARG, "weighted_i32: n=%lld", (long long)n);
  if (!cdf) return fail(HGNN_E_ARG, "weighted_i32: null cdf");
  if (int rc = guide_rule("weighted_i32", cdf, n_posts, T, guide, shift, n_guide)) return rc;
  if (!d_seed || !out) return fail(HGNN_E_ARG, "weighted_i32: null pointer");
  if (n == 0) return HGNN_OK;
  hipLaunchKernelGGL(k_weighted_i32, dim3((unsigned)cdiv(n, 256)), dim3(256), 0,
                     as_stream(stream), d_seed, n,
                     table_of(cdf, n_posts, T, guide, shift, n_guide), out);
  return check_launch("k_weighted_i32");
}

int hgnn_weighted_avoid_i32(const uint64_t* d_seed, int64_t n, int32_t n_neg, const int64_t* cdf,
                            int64_t n_posts, int64_t T, const int32_t* guide, int32_t shift,
                            int32_t n_guide, const int32_t* user_of_pos, int64_t n_users,
                            const int32_t* seen_rowptr, const int32_t* seen_col, int32_t tries,
                            int32_t* out, int64_t* d_kept_seen, hgnn_stream_t stream) {
  if (n < 0 || n_neg < 1 || n % n_neg)
    return fail(HGNN_E_ARG, "weighted_avoid_i32: n=%lld n_neg=%d", (long long)n, n_neg);
  if (tries < 1) return fail(HGNN_E_ARG, "weighted_avoid_i32: tries=%d", tries);
  if (n_users < 0) return fail(HGNN_E_ARG, "weighted_avoid_i32: n_users=%lld", (long long)n_users);
  if (int rc = guide_rule("weighted_avoid_i32", cdf, n_posts, T, guide, shift, n_guide)) return rc;
  if (!d_seed || !out || !user_of_pos || !seen_rowptr || !seen_col)
    return fail(HGNN_E_ARG, "weighted_avoid_i32: null pointer");
  if (n == 0) return HGNN_OK;
  hipLaunchKernelGGL(k_weighted_avoid_i32, dim3((unsigned)cdiv(n, 256)), dim3(256), 0,
                     as_stream(stream), d_seed, n, n_neg,
                     table_of(cdf, n_posts, T, guide, shift, n_guide), user_of_pos, n_users,
                     seen_rowptr, seen_col, tries, out,
                     reinterpret_cast<unsigned long long*>(d_kept_seen));
  return check_launch("k_weighted_avoid_i32");
}

}  // extern "C"
