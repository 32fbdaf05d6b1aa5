// A 64-bit checksum of a table's bit patterns, in one streaming pass.
//
// The layer-1 mean aggregates of a static input table are kept across steps (ops.gather_mean,
// static=True), keyed by the tensor's identity, pointer and version counter.  A native kernel
// that rewrites the table through a raw pointer bumps no version, so HGNN_STATIC_AGG=check keeps
// this checksum with each kept aggregate and recomputes it on every hit.
//
//   fp(x) = sum_i  bits(x[i]) * (K + 2 i)   (mod 2^64),   K = 0x9E3779B97F4A7C15
//
// Every multiplier is odd, so flipping any one bit of any word changes the sum; the multiplier
// depends on the index, so exchanging two unequal words changes it too.  Integer sums wrap and
// commute: the result does not depend on the order the blocks arrive in (no float atomics).
// One vector 64-bit atomicAdd per block.
#include "hgnn_common.h"

#include <algorithm>

namespace hgnn {

constexpr uint64_t kFpMul = 0x9E3779B97F4A7C15ull;
constexpr int kFpThreads = 256;
constexpr int kFpMaxBlocks = 256 * 8;   // 8 blocks of 4 waves per CU: a full chip of loads in flight

__device__ __forceinline__ uint64_t fp_term(uint32_t w, int64_t i) {
  return (uint64_t)w * (kFpMul + 2ull * (uint64_t)i);
}

// VEC: 16 B per lane (x 16-byte aligned); else 4 B per lane.  n: elements.
template <bool VEC>
__global__ void __launch_bounds__(kFpThreads) k_table_fingerprint(
    const uint32_t* __restrict__ x, int64_t n, unsigned long long* __restrict__ out) {
  uint64_t acc = 0;
  const int64_t tid = (int64_t)blockIdx.x * kFpThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kFpThreads;
  if constexpr (VEC) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const int64_t n4 = n >> 2;
    for (int64_t q = tid; q < n4; q += stride) {
      const u4 v = __builtin_nontemporal_load(reinterpret_cast<const u4*>(x) + q);
      const int64_t i = q << 2;
      acc += fp_term(v.x, i) + fp_term(v.y, i + 1) + fp_term(v.z, i + 2) + fp_term(v.w, i + 3);
    }
    const int64_t i = (n4 << 2) + tid;          // the tail: fewer than 4 words
    if (i < n) acc += fp_term(x[i], i);
  } else {
    for (int64_t i = tid; i < n; i += stride) acc += fp_term(x[i], i);
  }
  // wave sum by shuffles, then one LDS slot per wave
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1)
    acc += (uint64_t)__shfl_xor((unsigned long long)acc, m, kWave);
  __shared__ unsigned long long part[kFpThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kFpThreads / kWave; ++w) s += part[w];
    atomicAdd(out, s);
  }
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_table_fingerprint(const float* x, int64_t n_elems, uint64_t* d_out,
                           hgnn_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  if (n_elems < 0 || !d_out || (n_elems > 0 && !x))
    return fail(HGNN_E_ARG, "table_fingerprint: bad arguments");
  if (reinterpret_cast<uintptr_t>(d_out) % 8)
    return fail(HGNN_E_ARG, "table_fingerprint: d_out is not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(x) % 4)
    return fail(HGNN_E_ARG, "table_fingerprint: x is not 4-byte aligned");
  hipError_t e = hipMemsetAsync(d_out, 0, sizeof(uint64_t), stream);
  if (e != hipSuccess)
    return fail(HGNN_E_HIP, "table_fingerprint: memset: %s", hipGetErrorString(e));
  if (n_elems == 0) return HGNN_OK;
  const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0;
  const int64_t per_thread = vec ? 4 : 1;
  const unsigned grid = (unsigned)std::min<int64_t>(
      kFpMaxBlocks, std::max<int64_t>(1, cdiv(n_elems, kFpThreads * per_thread)));
  const uint32_t* xb = reinterpret_cast<const uint32_t*>(x);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(d_out);
  if (vec)
    hipLaunchKernelGGL(k_table_fingerprint<true>, dim3(grid), dim3(kFpThreads), 0, stream, xb,
                       n_elems, out);
  else
    hipLaunchKernelGGL(k_table_fingerprint<false>, dim3(grid), dim3(kFpThreads), 0, stream, xb,
                       n_elems, out);
  return check_launch("k_table_fingerprint");
}

}  // extern "C"
