// fp32 -> bf16 row cast of the opt-in bf16 row mode (HGNN_ROW_DTYPE=bf16): the shadow table the
// forward gathers and the link loss read in place of a layer output.  A streaming pass, 8
// elements per lane: two 16-B loads, one 16-B store.
//
// Round to nearest, ties to even, on the bit pattern (u + 0x7fff + the kept part's lowest bit,
// then the high half): exactly torch's float -> bfloat16 for every finite value and infinity,
// denormals included (bf16 has fp32's exponent range, so they round like any other value), and
// independent of the denormal mode a hardware convert would follow.  NaN becomes the quiet NaN
// 0x7fc0, as torch's does.
#include "hgnn_common.h"

namespace hgnn {

__device__ __forceinline__ uint32_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) {
  return bf16_rne(lo) | (bf16_rne(hi) << 16);
}

__global__ void __launch_bounds__(256) k_rows_to_bf16(const float* __restrict__ x, int64_t n,
                                                      uint16_t* __restrict__ out) {
  const int64_t n8 = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  uint4* o4 = reinterpret_cast<uint4*>(out);
  for (int64_t i = t; i < n8; i += stride) {
    const float4 a = x4[2 * i], b = x4[2 * i + 1];
    o4[i] = make_uint4(bf16_pack(a.x, a.y), bf16_pack(a.z, a.w), bf16_pack(b.x, b.y),
                       bf16_pack(b.z, b.w));
  }
  for (int64_t i = (n8 << 3) + t; i < n; i += stride)   // the n % 8 tail
    out[i] = (uint16_t)bf16_rne(x[i]);
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_rows_to_bf16(const float* x, int64_t n_elems, uint16_t* out, hgnn_stream_t stream_) {
  if (n_elems < 0) return fail(HGNN_E_ARG, "rows_to_bf16: n_elems=%lld", (long long)n_elems);
  if (n_elems == 0) return HGNN_OK;
  if (!x || !out) return fail(HGNN_E_ARG, "rows_to_bf16: null pointer");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15)
    return fail(HGNN_E_ARG, "rows_to_bf16: x and out must be 16-byte aligned");
  const int64_t blocks = std::min<int64_t>(cdiv(cdiv(n_elems, 8), 256), 8192);
  hipLaunchKernelGGL(k_rows_to_bf16, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream_), x,
                     n_elems, out);
  return check_launch("k_rows_to_bf16");
}

}  // extern "C"
