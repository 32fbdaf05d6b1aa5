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

// ReLU's backward fused into the cast (the opt-in bf16 gradient rows, HGNN_GRAD_ROW_DTYPE=bf16):
// dz = bf16(out > 0 ? dout : +0), the table a pre-projected relation's K2 reads, without the
// fp32 dz in between.  A masked element is +0 and a kept one dout's own bits (a NaN too), as the
// K3 backward kernels mask it, so the result is bitwise rows_to_bf16 of their dz_out.
__device__ __forceinline__ float keep_if(bool on, float v) { return on ? v : 0.f; }

__device__ __forceinline__ uint4 pack8(float4 a, float4 b) {
  return make_uint4(bf16_pack(a.x, a.y), bf16_pack(a.z, a.w), bf16_pack(b.x, b.y),
                    bf16_pack(b.z, b.w));
}

// The predicate from the forward's output: elementwise, n8 groups of 8 consecutive elements.
__global__ void __launch_bounds__(256) k_relu_grad_to_bf16_act(const float* __restrict__ dout,
                                                               const float* __restrict__ act,
                                                               int64_t n8,
                                                               uint16_t* __restrict__ dz) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float4* d4 = reinterpret_cast<const float4*>(dout);
  const float4* m4 = reinterpret_cast<const float4*>(act);
  uint4* o4 = reinterpret_cast<uint4*>(dz);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    float4 a = d4[2 * i], b = d4[2 * i + 1];
    const float4 ma = m4[2 * i], mb = m4[2 * i + 1];
    a.x = keep_if(ma.x > 0.f, a.x); a.y = keep_if(ma.y > 0.f, a.y);
    a.z = keep_if(ma.z > 0.f, a.z); a.w = keep_if(ma.w > 0.f, a.w);
    b.x = keep_if(mb.x > 0.f, b.x); b.y = keep_if(mb.y > 0.f, b.y);
    b.z = keep_if(mb.z > 0.f, b.z); b.w = keep_if(mb.w > 0.f, b.w);
    o4[i] = pack8(a, b);
  }
}

// The predicate from the bits hgnn_linear_fwd_mask wrote (linear_common.h): column j of a row is
// bit 4 (j / 16) + j % 4 of the row's word (j / 4) % 4; four words per row at every h.  L = h / 8
// lanes per row, and a wave takes 64 / L whole rows per step (its last 64 % L lanes idle where L
// is no power of two), so a row's lanes share a wave: lanes 0 and 1 of the row load its words
// {0, 1} and {2, 3}, 8 B each and 16 B per row in all, and lane q, whose columns 8 q .. 8 q + 7
// sit in words 2 (q & 1) and 2 (q & 1) + 1 at bits 4 (q / 2) .., takes them from lane q & 1.
__global__ void __launch_bounds__(256) k_relu_grad_to_bf16_bits(const float* __restrict__ dout,
                                                                const uint32_t* __restrict__ mask,
                                                                int64_t n_rows, int32_t L,
                                                                uint16_t* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int rows_w = 64 / L;                      // rows per wave step
  const int r = lane / L, q = lane - r * L;
  const bool mine = r < rows_w;
  const int from = r * L + (q & 1);               // the row's lane holding this lane's words
  const int shift = 4 * (q >> 1);
  const int64_t n_steps = (n_rows + rows_w - 1) / rows_w;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const float4* d4 = reinterpret_cast<const float4*>(dout);
  uint4* o4 = reinterpret_cast<uint4*>(dz);
  // (the loop bounds are wave-uniform: every lane reaches the shuffles of every step)
  for (int64_t s = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s < n_steps;
       s += waves) {
    const int64_t row = s * rows_w + r;
    const bool on = mine && row < n_rows;
    uint2 w = make_uint2(0u, 0u);
    if (on && q < 2) w = *reinterpret_cast<const uint2*>(mask + row * 4 + 2 * q);
    const uint32_t w0 = (uint32_t)__shfl((int)w.x, from) >> shift;
    const uint32_t w1 = (uint32_t)__shfl((int)w.y, from) >> shift;
    if (!on) continue;
    const int64_t i = row * L + q;
    float4 a = d4[2 * i], b = d4[2 * i + 1];
    a.x = keep_if(w0 & 1u, a.x); a.y = keep_if(w0 & 2u, a.y);
    a.z = keep_if(w0 & 4u, a.z); a.w = keep_if(w0 & 8u, a.w);
    b.x = keep_if(w1 & 1u, b.x); b.y = keep_if(w1 & 2u, b.y);
    b.z = keep_if(w1 & 4u, b.z); b.w = keep_if(w1 & 8u, b.w);
    o4[i] = pack8(a, b);
  }
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

int hgnn_relu_grad_to_bf16(const float* dout, const float* out_act, const uint32_t* mask,
                           int64_t n_rows, int32_t h, uint16_t* dz, hgnn_stream_t stream_) {
  if (n_rows < 0) return fail(HGNN_E_ARG, "relu_grad_to_bf16: n_rows=%lld", (long long)n_rows);
  if (h <= 0 || h % 8)
    return fail(HGNN_E_UNSUPPORTED, "relu_grad_to_bf16: h=%d must be a positive multiple of 8",
                (int)h);
  if (out_act && mask)
    return fail(HGNN_E_ARG, "relu_grad_to_bf16: both out_act and mask given (exactly one is the "
                            "ReLU predicate)");
  if (n_rows == 0) return HGNN_OK;
  if (!out_act && !mask)
    return fail(HGNN_E_ARG, "relu_grad_to_bf16: neither out_act nor mask given (exactly one is "
                            "the ReLU predicate)");
  if (!dout || !dz) return fail(HGNN_E_ARG, "relu_grad_to_bf16: null pointer");
  if ((reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(out_act) |
       reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(dz)) & 15)
    return fail(HGNN_E_ARG, "relu_grad_to_bf16: dout, out_act / mask and dz must be 16-byte "
                            "aligned");
  if (mask && (h % 16 || h > 128))
    return fail(HGNN_E_UNSUPPORTED, "relu_grad_to_bf16: h=%d has no bit form of the mask "
                                    "(h %% 16 == 0 and h <= 128); give out_act", (int)h);
  hipStream_t stream = as_stream(stream_);
  if (mask) {
    const int32_t L = h / 8;
    const int64_t steps = cdiv(n_rows, (int64_t)(64 / L));
    const int64_t blocks = std::min<int64_t>(cdiv(steps, 4), 8192);
    hipLaunchKernelGGL(k_relu_grad_to_bf16_bits, dim3((unsigned)blocks), dim3(256), 0, stream,
                       dout, mask, n_rows, L, dz);
    return check_launch("k_relu_grad_to_bf16_bits");
  }
  const int64_t n8 = n_rows * (int64_t)(h / 8);
  const int64_t blocks = std::min<int64_t>(cdiv(n8, 256), 8192);
  hipLaunchKernelGGL(k_relu_grad_to_bf16_act, dim3((unsigned)blocks), dim3(256), 0, stream, dout,
                     out_act, n8, dz);
  return check_launch("k_relu_grad_to_bf16_act");
}

}  // extern "C"
