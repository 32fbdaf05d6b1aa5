// K3/K4 on fp32 MFMA at compile-time shapes: the persistent v4 / v5 kernels and their launchers.
// (linear.hip: what K3 computes, and which family a call takes; linear_general.hip: the MFMA
// operand layout these kernels share.)
#include "linear_common.h"

#include <algorithm>

namespace hgnn {

// ================================================================ v4: compile-time shapes
// H (output width) in {64, 128}, K (sum of segments) in {64, 128, 256}, every segment a multiple
// of 16 columns and float4-aligned.  Per 16-column chunk c of the concatenated input, a host-built
// table gives the segment base/stride (no per-element segment search).
// LDS strides are chosen so that addresses stay affine in the lane id (the compiler keeps one
// base register + immediates) and the two access kinds are conflict-free:
//   * ds_read_b128 where lanes (i, g) read row i, columns 4g..4g+3: stride = 8 (mod 16) dwords
//     (row i lands on 16-B slot 2i + g: even/odd by g, 8 distinct per b128 lane group);
//   * ds_read_b32 where lanes (i, g) read row g, column i: stride = 16 (mod 32) dwords.

// Address of row `row`'s float4 at columns 16 c + 4 g .. +3 of the concatenated input.  S8: every
// 8 consecutive chunks are one segment (segments 128 columns wide, as at cfg3/cfg4), so with c
// unrolled the row offset is one multiply per segment and the chunks are immediates off it
// (the general form keeps a 64-bit address per chunk live across the MFMA sweep).
template <bool S8>
__device__ __forceinline__ const float4* x_chunk(const ChunkTab& tab, int64_t row, int c, int g) {
  if constexpr (S8) {
    const int s = c & ~7;
    return reinterpret_cast<const float4*>(tab.x[s] + row * tab.ld[s] + tab.col[s] +
                                           (c & 7) * 16 + 4 * g);
  } else {
    return reinterpret_cast<const float4*>(tab.x[c] + row * tab.ld[c] + tab.col[c] + 4 * g);
  }
}

// The added rows of one 16-row tile (hgnn_linear_fwd_add: a pre-projected relation's gathered
// mean), loaded before the tile's MFMA sweep, which hides their HBM latency; read in the
// epilogue they stalled every tile (K = 128 + add ran at 0.53 of the fp32 MFMA peak).  Lane
// (i, g) holds columns 16 tt + 4 g .. +3 of its row.  The bias stays an epilogue read (L1-hot).
template <int NT, bool ADD>
struct Epi {
  float4 d[ADD ? NT : 1];
  __device__ __forceinline__ void load(const LinArgs& a, int64_t row, int H, int g) {
    if constexpr (ADD) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
        d[tt] = row < a.n ? *reinterpret_cast<const float4*>(a.add + row * H + tt * 16 + 4 * g)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // (acc + bias) + add: the order of the unfused expression
  __device__ __forceinline__ float4 sum(const f32x4& acc, int tt, const LinArgs& a, int g) const {
    const float4 bb = a.bias ? *reinterpret_cast<const float4*>(a.bias + tt * 16 + 4 * g)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = make_float4(acc[0] + bb.x, acc[1] + bb.y, acc[2] + bb.z, acc[3] + bb.w);
    if constexpr (ADD) {
      v.x += d[tt].x; v.y += d[tt].y; v.z += d[tt].z; v.w += d[tt].w;
    }
    return v;
  }
};

// Forward v4: persistent.  W is staged into LDS once per block; then each of the 8 waves streams
// its own 16-row tiles (no further barriers), with the next tile's A fragments in flight during
// the current tile's MFMAs.  (Measured and rejected: MFMAs interleaved across accumulators —
// the 4-deep dependent chains are already covered by 4 waves per SIMD — and a two-stage register
// ping-pong instead of the copy, which spills: 193-200 us vs 202-205 and 227 at N=1M, K=128.)  Output tiles are computed transposed (out^T = W X^T) so every lane
// stores one float4 per 16 output columns.
template <int H, int K, bool ADD, bool S8 = false>
__global__ void __launch_bounds__(512, (H <= 64 && K <= 128 ? 4 : (K <= 128 ? 3 : 2))) k_linear_fwd_v4(const LinArgs a, const ChunkTab tab,
                                                       int64_t n_tiles) {
  constexpr int NT = H / 16, KC = K / 16, LDW = K + 8;
  __shared__ __attribute__((aligned(16))) float ws[H * LDW];
  for (int idx = threadIdx.x; idx < H * K / 4; idx += 512) {
    const int j = idx / (K / 4), k = (idx % (K / 4)) * 4;
    *reinterpret_cast<float4*>(ws + j * LDW + k) =
        *reinterpret_cast<const float4*>(a.w + (int64_t)j * K + k);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t nw = (int64_t)gridDim.x * 8;
  auto load = [&](int64_t t, float4 (&v)[KC]) {
    const int64_t row = t * 16 + i;
#pragma unroll
    for (int c = 0; c < KC; ++c)
      v[c] = row < a.n ? *x_chunk<S8>(tab, row, c, g) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  int64_t t = (int64_t)blockIdx.x * 8 + wave;
  float4 av[KC], an[KC];
  if (t < n_tiles) load(t, av);
  __syncthreads();
  const int wl0 = i * LDW + 4 * g;
  for (; t < n_tiles; t += nw) {
    if (t + nw < n_tiles) load(t + nw, an);
    // opaque offset: keeps the loop-invariant W fragments as per-tile LDS reads instead of letting
    // the compiler hoist all K*H/64 of them into VGPRs (measured 195 vs 204 us at N=1M, K=128, H=64,
    // and no spill at H=128)
    int wo = wl0;
    asm volatile("" : "+v"(wo));
    const float* wl = ws + wo;
    const int64_t row = t * 16 + i;
    Epi<NT, ADD> ep;               // the added rows, in flight during the sweep
    ep.load(a, row, H, g);
    f32x4 acc[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const float4 bv = *reinterpret_cast<const float4*>(wl + tt * 16 * LDW + c * 16);
        acc[tt] = mfma4(bv.x, av[c].x, acc[tt]);
        acc[tt] = mfma4(bv.y, av[c].y, acc[tt]);
        acc[tt] = mfma4(bv.z, av[c].z, acc[tt]);
        acc[tt] = mfma4(bv.w, av[c].w, acc[tt]);
      }
    if (row < a.n) {
      uint32_t mbits = 0;   // ReLU mask bits of this lane's columns (mask_out)
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        float4 v = ep.sum(acc[tt], tt, a, g);
        if (a.relu) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        mbits |= relu_bits(v, 4 * tt);
        *reinterpret_cast<float4*>(a.out + row * H + tt * 16 + 4 * g) = v;
      }
      if (a.mask_out) a.mask_out[row * 4 + g] = mbits;
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) av[c] = an[c];
  }
}

// Backward v4: two roles per SIMD.  512 threads; waves 0-3 ("dz waves") load the masked dz
// fragments of 16 rows each, run dgrad (dX^T = W^T dz^T, straight from registers) and the bias
// sums, and publish dz to LDS; waves 4-7 ("X waves") stage the X tile and run wgrad.  dz / X
// tiles are double-buffered, so with one barrier per tile the dgrad of tile t+1 (dz waves) runs
// beside the wgrad of tile t (X waves) on every SIMD: MFMA issue from one role hides the memory
// waits of the other.
// T = 32 (wgrad-only, for K = 256 whose X tiles would not fit twice at T = 64): the two 16-row
// slices of a tile go to dz waves (w & 1), each loading half of the columns (w >> 1).
template <int H, int K, bool DX, int T = 64>
__global__ void __launch_bounds__(512) k_linear_bwd_v4(const LinArgs a, const ChunkTab tab,
                                                       int64_t n_tiles) {
  static_assert(T == 64 || (T == 32 && !DX), "dgrad needs one 16-row slice per dz wave");
  constexpr int HC = H / 16, KC = K / 16;
  constexpr int ZR = T / 16;                // 16-row slices per tile
  constexpr int ZC = HC * ZR / 4;           // column chunks loaded per dz wave
  constexpr int JT = H / 64;                // wgrad j tiles per X wave
  constexpr int XQ = T * K / 4 / 256;       // X float4 per X-wave thread per tile
  constexpr int LWT = H + 8, LZ = H + 16, LX = K + 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wt = smem;                         // [K][LWT]  W^T   (DX only)
  float* dzb = wt + (DX ? K * LWT : 0);     // 2 x [T][LZ]
  float* xsb = dzb + 2 * T * LZ;            // 2 x [T][LX]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const bool zrole = wave < 4;
  const int w4 = wave & 3;
  const int zrow = w4 % ZR, zcol0 = (w4 / ZR) * ZC;   // dz wave: row slice, first column chunk
  if (DX) {
    for (int idx = threadIdx.x; idx < H * K; idx += 512) {
      const int j = idx / K, k = idx % K;
      wt[k * LWT + j] = a.w[(int64_t)j * K + k];
    }
    __syncthreads();   // block-uniform: W^T image complete before the first dgrad
  }
  const int64_t n_my = (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x;
  if (zrole) {
    auto load_dz = [&](int64_t it, float4 (&z)[HC]) {
      const int64_t row = (blockIdx.x + it * gridDim.x) * T + zrow * 16 + i;
      const uint32_t mk = a.mask_in && it < n_my && row < a.n ? a.mask_in[row * 4 + g] : 0u;
#pragma unroll
      for (int c = 0; c < HC; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (it < n_my && row < a.n && c >= zcol0 && c < zcol0 + ZC) {
          v = *reinterpret_cast<const float4*>(a.dout + row * H + c * 16 + 4 * g);
          if (a.mask_in) {
            v = mask4(v, mk, 4 * c);
          } else if (a.out_act) {
            const float4 m =
                *reinterpret_cast<const float4*>(a.out_act + row * H + c * 16 + 4 * g);
            v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
            v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
          }
        }
        z[c] = v;
      }
    };
    float4 dbacc[HC], zc[HC], zn[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) dbacc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    load_dz(0, zc);
    const float* wt_r = wt + i * LWT + 4 * g;
    for (int64_t it = 0; it <= n_my; ++it) {
      if (it < n_my) {
        // dz tile element (r, c) lives at r * LZ + (c ^ (((r >> 2) & 3) << 2)): the float4 writes
        // here (lane (i, g): row 16 zrow + i, 16-B slot g of each chunk) and the b32 column reads of
        // the X waves (lane (i, g): row 4 s + g, column 16 J + i) both hit 64 distinct banks
        float* dz_w = dzb + (it & 1) * T * LZ + (zrow * 16 + i) * LZ + 4 * (g ^ ((i >> 2) & 3));
        if (a.dz_out) {
          const int64_t row = (blockIdx.x + it * gridDim.x) * T + zrow * 16 + i;
          if (row < a.n) {
#pragma unroll
            for (int c = 0; c < HC; ++c)
              if (c >= zcol0 && c < zcol0 + ZC)
                *reinterpret_cast<float4*>(a.dz_out + row * H + c * 16 + 4 * g) = zc[c];
          }
        }
#pragma unroll
        for (int c = 0; c < HC; ++c) {
          if (c >= zcol0 && c < zcol0 + ZC) *reinterpret_cast<float4*>(dz_w + c * 16) = zc[c];
          dbacc[c].x += zc[c].x; dbacc[c].y += zc[c].y;
          dbacc[c].z += zc[c].z; dbacc[c].w += zc[c].w;
        }
        load_dz(it + 1, zn);
        if (DX) {
          const int64_t row = (blockIdx.x + it * gridDim.x) * T + zrow * 16 + i;
#pragma unroll
          for (int ct = 0; ct < KC; ct += 2) {
            f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
            for (int c = 0; c < HC; ++c) {
              const float4 b0 = *reinterpret_cast<const float4*>(wt_r + ct * 16 * LWT + c * 16);
              const float4 b1 =
                  *reinterpret_cast<const float4*>(wt_r + (ct + 1) * 16 * LWT + c * 16);
              o0 = mfma4(b0.x, zc[c].x, o0); o1 = mfma4(b1.x, zc[c].x, o1);
              o0 = mfma4(b0.y, zc[c].y, o0); o1 = mfma4(b1.y, zc[c].y, o1);
              o0 = mfma4(b0.z, zc[c].z, o0); o1 = mfma4(b1.z, zc[c].z, o1);
              o0 = mfma4(b0.w, zc[c].w, o0); o1 = mfma4(b1.w, zc[c].w, o1);
            }
            if (row < a.n) {
#pragma unroll
              for (int h2 = 0; h2 < 2; ++h2) {
                float* dx = tab.dx[ct + h2];
                if (dx) {
                  const f32x4 o = h2 ? o1 : o0;
                  store_dx4(dx + row * tab.ld[ct + h2] + tab.col[ct + h2] + 4 * g,
                            (tab.dx_acc >> (ct + h2)) & 1u, o[0], o[1], o[2], o[3]);
                }
              }
            }
          }
        }
#pragma unroll
        for (int c = 0; c < HC; ++c) zc[c] = zn[c];
      }
      __syncthreads();
    }
    // bias: reduce over i (16 lanes), then over the 4 dz waves through LDS (fixed order)
    float* red = xsb;   // X buffers are idle after the final barrier of the X waves below
    __syncthreads();
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      float4 v = dbacc[c];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        v.x += __shfl_xor(v.x, m, 64); v.y += __shfl_xor(v.y, m, 64);
        v.z += __shfl_xor(v.z, m, 64); v.w += __shfl_xor(v.w, m, 64);
      }
      if (i == 0) *reinterpret_cast<float4*>(red + w4 * H + c * 16 + 4 * g) = v;
    }
    __syncthreads();
  } else {
    constexpr int XR = 256 / (K / 4);
    const int t4 = threadIdx.x - 256;
    const int xq_col = (t4 % (K / 4)) * 4, xq_row0 = t4 / (K / 4);
    const int xc = xq_col / 16;
    const float* xseg = tab.x[xc] + tab.col[xc] + (xq_col % 16);
    const int xld = tab.ld[xc];
    auto load_x = [&](int64_t it, float4 (&x)[XQ]) {
      const int64_t r0 = (blockIdx.x + it * gridDim.x) * T;
#pragma unroll
      for (int q = 0; q < XQ; ++q) {
        const int64_t row = r0 + xq_row0 + q * XR;
        x[q] = (it < n_my && row < a.n) ? *reinterpret_cast<const float4*>(xseg + row * xld)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    f32x4 wacc[JT][KC];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int kt = 0; kt < KC; ++kt) wacc[jt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 xp[XQ];
    load_x(0, xp);
    for (int64_t it = 0; it <= n_my; ++it) {
      if (it < n_my) {
        float* xs_w = xsb + (it & 1) * T * LX + xq_row0 * LX + xq_col;
#pragma unroll
        for (int q = 0; q < XQ; ++q) *reinterpret_cast<float4*>(xs_w + q * XR * LX) = xp[q];
        load_x(it + 1, xp);
      }
      if (it >= 1) {   // wgrad of tile it-1 (its dz / X buffers were completed last barrier)
        const int b = (it - 1) & 1;
        const float* dz_r = dzb + b * T * LZ + g * LZ + (w4 * JT) * 16;
        const float* xs_r = xsb + b * T * LX + g * LX + i;
#pragma unroll 4
        for (int s4 = 0; s4 < T / 4; ++s4) {
          float az[JT];
#pragma unroll
          for (int jt = 0; jt < JT; ++jt)
            az[jt] = dz_r[s4 * 4 * LZ + jt * 16 + (i ^ ((s4 & 3) << 2))];   // swizzled (above)
#pragma unroll
          for (int kt = 0; kt < KC; ++kt) {
            const float bx = xs_r[s4 * 4 * LX + kt * 16];
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) wacc[jt][kt] = mfma4(az[jt], bx, wacc[jt][kt]);
          }
        }
      }
      __syncthreads();
    }
    constexpr int KEXT = K + 1;
    float* slab = a.slab + (int64_t)blockIdx.x * H * KEXT;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int kt = 0; kt < KC; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          slab[(int64_t)((w4 * JT + jt) * 16 + 4 * g + r) * KEXT + kt * 16 + i] =
              wacc[jt][kt][r];
    __syncthreads();
    __syncthreads();
  }
  // both roles passed the same number of barriers (n_my + 1, then 2)
  if (threadIdx.x < H) {
    const float* red = xsb;
    a.slab[(int64_t)blockIdx.x * H * (K + 1) + (int64_t)threadIdx.x * (K + 1) + K] =
        ((red[threadIdx.x] + red[H + threadIdx.x]) + red[2 * H + threadIdx.x]) +
        red[3 * H + threadIdx.x];
  }
}

// Weight gradient alone, v5: dW = dz^T [X_0 .. X_{S-1}] and db = colsum(dz), dz = dout * [out > 0].
// Persistent 512-thread blocks; every wave stages a share of each T-row tile (masked dz and X,
// float4 loads issued one tile ahead into registers) into double-buffered LDS, one barrier per
// tile, and EVERY wave runs MFMAs on the tile (v4's wgrad-only variant left the four dz-loading
// waves without MFMA work: one MFMA wave per SIMD).  Wave w owns 2 j-tiles x KW k-tiles of the
// [H][K] output: per 4-row k-step 2 + KW b32 LDS reads feed 2 KW independent MFMAs.  Row strides
// H+16 / K+16 keep the b32 reads conflict-free.  The block's partial dW/db goes to its slab
// (k_wgrad_reduce sums the slabs in block order: deterministic).
template <int H, int K, int T>
__global__ void __launch_bounds__(512) k_linear_wgrad_v5(const LinArgs a, const ChunkTab tab,
                                                         int64_t n_tiles) {
  constexpr int HC = H / 16, KC = K / 16;
  constexpr int JG = HC / 2;                 // j-tile pairs
  constexpr int KG = 8 / JG;                 // k groups per j pair (8 waves)
  constexpr int KW = KC / KG;                // k tiles per wave
  static_assert(JG * KG == 8 && KW * KG == KC, "wave split");
  constexpr int LZ = H + 16, LX = K + 16;
  constexpr int ZQ = T * H / 4 / 512;        // dz float4 per thread per tile
  constexpr int XQ = T * K / 4 / 512;        // X float4 per thread per tile
  static_assert(ZQ >= 1 && XQ >= 1, "tile too small for 512 threads");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dzb = smem;                         // 2 x [T][LZ]
  float* xsb = dzb + 2 * T * LZ;             // 2 x [T][LX]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int jt0 = 2 * (wave / KG), kt0 = (wave % KG) * KW;
  // fixed staging columns per thread (H/4 and K/4 divide 512)
  const int zc4 = threadIdx.x % (H / 4), zr0 = threadIdx.x / (H / 4);
  constexpr int ZR = 512 / (H / 4);          // rows apart between a thread's dz float4
  const int xk4 = threadIdx.x % (K / 4), xr0 = threadIdx.x / (K / 4);
  constexpr int XR = 512 / (K / 4);
  const int xc = xk4 / 4;
  const float* xseg = tab.x[xc] + tab.col[xc] + 4 * (xk4 % 4);
  const int xld = tab.ld[xc];
  const bool bits = a.mask_in != nullptr;
  const bool masked = !bits && a.out_act != nullptr;
  const int64_t n_my = (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x;
  const int64_t last = a.n - 1;
  float4 zp[ZQ], mp[ZQ], xp[XQ];
  uint32_t bp[ZQ];
  const int bshift = 4 * (zc4 >> 2);        // columns 4 zc4 .. +3: chunk zc4/4, lane group zc4%4
  auto issue = [&](int64_t it) {
    const int64_t r0 = (blockIdx.x + it * gridDim.x) * T;
#pragma unroll
    for (int q = 0; q < ZQ; ++q) {
      const int64_t row = min<int64_t>(r0 + zr0 + q * ZR, last);
      zp[q] = *reinterpret_cast<const float4*>(a.dout + row * H + 4 * zc4);
      if (bits) bp[q] = a.mask_in[row * 4 + (zc4 & 3)];
      if (masked) mp[q] = *reinterpret_cast<const float4*>(a.out_act + row * H + 4 * zc4);
    }
#pragma unroll
    for (int q = 0; q < XQ; ++q) {
      const int64_t row = min<int64_t>(r0 + xr0 + q * XR, last);
      xp[q] = *reinterpret_cast<const float4*>(xseg + row * xld);
    }
  };
  f32x4 acc[2][KW];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[j][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n_my > 0) issue(0);
  for (int64_t it = 0; it < n_my; ++it) {
    const int b = it & 1;
    const int64_t r0 = (blockIdx.x + it * gridDim.x) * T;
    float* dz_w = dzb + b * T * LZ;
    float* xs_w = xsb + b * T * LX;
#pragma unroll
    for (int q = 0; q < ZQ; ++q) {
      const int r = zr0 + q * ZR;
      float4 v = zp[q];
      if (bits) v = mask4(v, bp[q], bshift);
      if (masked) {
        v.x = mp[q].x > 0.f ? v.x : 0.f; v.y = mp[q].y > 0.f ? v.y : 0.f;
        v.z = mp[q].z > 0.f ? v.z : 0.f; v.w = mp[q].w > 0.f ? v.w : 0.f;
      }
      if (r0 + r >= a.n) v = make_float4(0.f, 0.f, 0.f, 0.f);   // clamped rows contribute 0
      dbacc.x += v.x; dbacc.y += v.y; dbacc.z += v.z; dbacc.w += v.w;
      *reinterpret_cast<float4*>(dz_w + r * LZ + 4 * zc4) = v;
    }
#pragma unroll
    for (int q = 0; q < XQ; ++q)
      *reinterpret_cast<float4*>(xs_w + (xr0 + q * XR) * LX + 4 * xk4) = xp[q];
    if (it + 1 < n_my) issue(it + 1);
    __syncthreads();
    const float* dz_r = dz_w + g * LZ + jt0 * 16 + i;
    const float* xs_r = xs_w + g * LX + kt0 * 16 + i;
#pragma unroll 4
    for (int s4 = 0; s4 < T / 4; ++s4) {
      const float a0 = dz_r[s4 * 4 * LZ], a1 = dz_r[s4 * 4 * LZ + 16];
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const float bx = xs_r[s4 * 4 * LX + k * 16];
        acc[0][k] = mfma4(a0, bx, acc[0][k]);
        acc[1][k] = mfma4(a1, bx, acc[1][k]);
      }
    }
  }
  constexpr int KEXT = K + 1;
  float* slab = a.slab + (int64_t)blockIdx.x * H * KEXT;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[(int64_t)((jt0 + j) * 16 + 4 * g + r) * KEXT + (kt0 + k) * 16 + i] = acc[j][k][r];
  // db: thread partials (fixed column 4*zc4) reduced through LDS in a fixed order
  __syncthreads();
  float4* red = reinterpret_cast<float4*>(smem);
  red[threadIdx.x] = dbacc;
  __syncthreads();
  if (threadIdx.x < H / 4) {
    float4 t = red[threadIdx.x];
    for (int m = threadIdx.x + H / 4; m < 512; m += H / 4) {
      const float4 u = red[m];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    const int c = threadIdx.x * 4;
    slab[(int64_t)(c + 0) * KEXT + K] = t.x;
    slab[(int64_t)(c + 1) * KEXT + K] = t.y;
    slab[(int64_t)(c + 2) * KEXT + K] = t.z;
    slab[(int64_t)(c + 3) * KEXT + K] = t.w;
  }
}

static size_t wgrad5_lds(int h, int k, int t) {
  return std::max<size_t>(((size_t)2 * t * (h + 16) + (size_t)2 * t * (k + 16)) * 4, 512 * 16);
}

static size_t v4_bwd_lds(int h, int k, bool dx, int t = 64) {
  return ((dx ? (size_t)k * (h + 8) : 0) + (size_t)2 * t * (h + 16) + (size_t)2 * t * (k + 16)) *
         4;
}

// dgrad alone, persistent: dX = (dout * [out > 0]) W with W^T staged in LDS once per block
// ([K][H+8], conflict-free b128 fragments); each of the 8 waves streams its own 16-row tiles with
// the next tile's masked dz fragments in flight, and computes dX^T = W^T dz^T so that every lane
// stores float4 runs of its row.  Used with the wgrad-only kernel when the fused backward's LDS
// (W^T + two dz and X tiles) does not fit: K = 256, or H = 128 with K = 128.
template <int H, int K>
__global__ void __launch_bounds__(512) k_linear_dgrad_v4(const LinArgs a, const ChunkTab tab,
                                                         int64_t n_tiles) {
  constexpr int HC = H / 16, KC = K / 16, LWT = H + 8;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wt = smem;   // [K][LWT]
  for (int idx = threadIdx.x; idx < H * K; idx += 512) {
    const int j = idx / K, k = idx % K;
    wt[k * LWT + j] = a.w[(int64_t)j * K + k];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t nw = (int64_t)gridDim.x * 8;
  auto load_dz = [&](int64_t t, float4 (&z)[HC]) {
    const int64_t row = t * 16 + i;
    const uint32_t mk = a.mask_in && row < a.n ? a.mask_in[row * 4 + g] : 0u;
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < a.n) {
        v = *reinterpret_cast<const float4*>(a.dout + row * H + c * 16 + 4 * g);
        if (a.mask_in) {
          v = mask4(v, mk, 4 * c);
        } else if (a.out_act) {
          const float4 m = *reinterpret_cast<const float4*>(a.out_act + row * H + c * 16 + 4 * g);
          v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
          v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
        }
      }
      z[c] = v;
    }
  };
  int64_t t = (int64_t)blockIdx.x * 8 + wave;
  float4 zc[HC], zn[HC];
  if (t < n_tiles) load_dz(t, zc);
  __syncthreads();
  const int wr0 = i * LWT + 4 * g;
  for (; t < n_tiles; t += nw) {
    if (t + nw < n_tiles) load_dz(t + nw, zn);
    int wo = wr0;
    asm volatile("" : "+v"(wo));   // keep W^T fragments as per-tile LDS reads (see fwd v4)
    const float* wt_r = wt + wo;
    const int64_t row = t * 16 + i;
    if (a.dz_out && row < a.n) {
#pragma unroll
      for (int c = 0; c < HC; ++c)
        *reinterpret_cast<float4*>(a.dz_out + row * H + c * 16 + 4 * g) = zc[c];
    }
#pragma unroll
    for (int ct = 0; ct < KC; ct += 2) {
      f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
      for (int c = 0; c < HC; ++c) {
        const float4 b0 = *reinterpret_cast<const float4*>(wt_r + ct * 16 * LWT + c * 16);
        const float4 b1 = *reinterpret_cast<const float4*>(wt_r + (ct + 1) * 16 * LWT + c * 16);
        o0 = mfma4(b0.x, zc[c].x, o0); o1 = mfma4(b1.x, zc[c].x, o1);
        o0 = mfma4(b0.y, zc[c].y, o0); o1 = mfma4(b1.y, zc[c].y, o1);
        o0 = mfma4(b0.z, zc[c].z, o0); o1 = mfma4(b1.z, zc[c].z, o1);
        o0 = mfma4(b0.w, zc[c].w, o0); o1 = mfma4(b1.w, zc[c].w, o1);
      }
      if (row < a.n) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          float* dx = tab.dx[ct + h2];
          if (dx) {
            const f32x4 o = h2 ? o1 : o0;
            store_dx4(dx + row * tab.ld[ct + h2] + tab.col[ct + h2] + 4 * g,
                      (tab.dx_acc >> (ct + h2)) & 1u, o[0], o[1], o[2], o[3]);
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < HC; ++c) zc[c] = zn[c];
  }
}

static size_t dgrad4_lds(int h, int k) { return (size_t)k * (h + 8) * 4; }

// dgrad v5: v4's tiling and W^T image, reorganised for 2 waves per SIMD: G column
// tiles in flight (G independent accumulators, k-step-major), W^T fragments read one k-sweep ahead
// (across column-group boundaries too), and the next tile's raw dout / out fragments held as
// loaded — the ReLU mask is applied when the tile becomes current, so no load is waited for at
// issue.  Rows past the end are clamped (loaded, never stored).
template <int H, int K>
__global__ void __launch_bounds__(512, 2) k_linear_dgrad_v5(const LinArgs a, const ChunkTab tab,
                                                            int64_t n_tiles) {
  constexpr int HC = H / 16, KC = K / 16, LWT = H + 8;
  constexpr int G = KC < 8 ? KC : 8, NG = KC / G;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wt = smem;   // [K][LWT]
  for (int idx = threadIdx.x; idx < H * K; idx += 512) {
    const int j = idx / K, k = idx % K;
    wt[k * LWT + j] = a.w[(int64_t)j * K + k];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t nw = (int64_t)gridDim.x * 8;
  const int64_t last = a.n - 1;
  const bool bits = a.mask_in != nullptr;
  const bool masked = !bits && a.out_act != nullptr;
  float4 zr[HC], mr[HC];
  uint32_t mk = 0u;
  auto issue = [&](int64_t t) {
    const int64_t row = min<int64_t>(t * 16 + i, last);
    if (bits) mk = a.mask_in[row * 4 + g];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      zr[c] = *reinterpret_cast<const float4*>(a.dout + row * H + c * 16 + 4 * g);
      if (masked) mr[c] = *reinterpret_cast<const float4*>(a.out_act + row * H + c * 16 + 4 * g);
    }
  };
  int64_t t = (int64_t)blockIdx.x * 8 + wave;
  if (t < n_tiles) issue(t);
  __syncthreads();
  const int wr0 = i * LWT + 4 * g;
  for (; t < n_tiles; t += nw) {
    float4 zc[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      zc[c] = zr[c];
      if (bits) zc[c] = mask4(zc[c], mk, 4 * c);
      if (masked) {
        zc[c].x = mr[c].x > 0.f ? zc[c].x : 0.f; zc[c].y = mr[c].y > 0.f ? zc[c].y : 0.f;
        zc[c].z = mr[c].z > 0.f ? zc[c].z : 0.f; zc[c].w = mr[c].w > 0.f ? zc[c].w : 0.f;
      }
    }
    issue(t + nw < n_tiles ? t + nw : t);
    int wo = wr0;
    asm volatile("" : "+v"(wo));   // keep W^T fragments as per-tile LDS reads (see fwd v4)
    const float* wt_r = wt + wo;
    const int64_t row = t * 16 + i;
    if (a.dz_out && row < a.n) {
#pragma unroll
      for (int c = 0; c < HC; ++c)
        *reinterpret_cast<float4*>(a.dz_out + row * H + c * 16 + 4 * g) = zc[c];
    }
    float4 bw[G];
#pragma unroll
    for (int j = 0; j < G; ++j) bw[j] = *reinterpret_cast<const float4*>(wt_r + j * 16 * LWT);
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      f32x4 o[G];
#pragma unroll
      for (int j = 0; j < G; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < HC; ++c) {
#pragma unroll
        for (int j = 0; j < G; ++j) o[j] = mfma4(bw[j].x, zc[c].x, o[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) o[j] = mfma4(bw[j].y, zc[c].y, o[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) o[j] = mfma4(bw[j].z, zc[c].z, o[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) {
          o[j] = mfma4(bw[j].w, zc[c].w, o[j]);
          if (c + 1 < HC)
            bw[j] = *reinterpret_cast<const float4*>(wt_r + (gi * G + j) * 16 * LWT + (c + 1) * 16);
          else if (gi + 1 < NG)
            bw[j] = *reinterpret_cast<const float4*>(wt_r + ((gi + 1) * G + j) * 16 * LWT);
        }
      }
      if (row < a.n) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const int ct = gi * G + j;
          float* dx = tab.dx[ct];
          if (dx)
            store_dx4(dx + row * tab.ld[ct] + tab.col[ct] + 4 * g, (tab.dx_acc >> ct) & 1u,
                      o[j][0], o[j][1], o[j][2], o[j][3]);
        }
      }
    }
  }
}

// ================================================================ launchers
// persistent grids: one block per CU, or two where two blocks' LDS fits a CU
constexpr int64_t kBlocks = 256;
constexpr size_t kLdsPerCu = 160 * 1024;
static int64_t blocks_per_cu(size_t lds) {
  return (int64_t)std::max<size_t>(1, std::min<size_t>(2, kLdsPerCu / lds));
}

// X(H, K) for the (h, K) of the call: the family's six shapes
#define HGNN_V4_SHAPES(X)            \
  switch (h * 1000 + K) {            \
    case 64064: X(64, 64); break;    \
    case 64128: X(64, 128); break;   \
    case 64256: X(64, 256); break;   \
    case 128064: X(128, 64); break;  \
    case 128128: X(128, 128); break; \
    default: X(128, 256); break;     \
  }

// every 8 consecutive 16-column chunks one 128-column segment (x_chunk<true>'s addressing)
static bool chunks_in_segments_of_8(const ChunkTab& tab, int k_total) {
  for (int c = 0; c < k_total / 16; ++c) {
    const int s = c & ~7;
    if (tab.x[c] != tab.x[s] || tab.ld[c] != tab.ld[s] || tab.col[c] != tab.col[s] + (c & 7) * 16)
      return false;
  }
  return true;
}

// the persistent forward also takes K = 256 (W: H*(K+8)*4 <= 135 KB of LDS, one block per CU)
int v4_linear_fwd(const LinArgs& a, const ChunkTab& tab, hipStream_t stream) {
  const int h = a.h, K = a.k_total;
  const int64_t n_tiles = cdiv(a.n, 16);
  const int64_t per_cu = blocks_per_cu((size_t)h * (K + 8) * 4);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n_tiles, 8),
                                                                    kBlocks * per_cu))),
      block(512);
  // 128-column segment addressing where every 8 chunks are one segment (round 3: -2.5 % at
  // K = 128, -1 % at K = 256 on the cfg4 shapes; the v5 schedule measured slower with it and
  // is no longer built)
  const bool s8 = h == 128 && K >= 128 && chunks_in_segments_of_8(tab, K);
#define HGNN_FWD4A(HV, KV, AV)                                                                    \
  if (s8) hipLaunchKernelGGL((k_linear_fwd_v4<HV, KV, AV, (HV == 128 && KV >= 128)>), grid, block, \
                             0, stream, a, tab, n_tiles);                                        \
  else hipLaunchKernelGGL((k_linear_fwd_v4<HV, KV, AV, false>), grid, block, 0, stream, a, tab,  \
                          n_tiles);
#define HGNN_FWD4(HV, KV) \
  if (a.add) { HGNN_FWD4A(HV, KV, true) } else { HGNN_FWD4A(HV, KV, false) }
  HGNN_V4_SHAPES(HGNN_FWD4)
#undef HGNN_FWD4
#undef HGNN_FWD4A
  return check_launch("k_linear_fwd_v4");
}

int64_t v4_bwd_max_slabs() { return kBlocks * 2; }

// fused two-role backward when W^T and two dz / X tiles fit the LDS; otherwise persistent
// dgrad + wgrad-only (T = 32 tiles for K = 256)
int v4_linear_bwd(LinArgs a, const ChunkTab& tab, bool dx, bool wg, void* ws, size_t ws_bytes,
                  int64_t* slabs, hipStream_t stream) {
  const int h = a.h, K = a.k_total;
  // H = K = 128: persistent dgrad v5 + wgrad v5 (T = 16) beat the fused two-role kernel
  // (6.21 vs 8.29 ms at N = 9M); H = 64, K = 128: the fused kernel wins (3.18 vs 3.94 ms)
  const bool split = h == 128 && K == 128;
  const bool fused = !split && dx && wg && K <= 128 && v4_bwd_lds(h, K, true) <= kLdsPerCu;
  if (dx && !fused) {
    const int64_t n16 = cdiv(a.n, 16);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n16, 8), kBlocks))),
        block(512);
    const size_t lds = dgrad4_lds(h, K);
    // v5 at H = 128 (K = 256: 5.06 vs 5.70 ms; K = 128: 3.22 vs 3.25 ms at N = 9M), v4 at H = 64
#define HGNN_DG4(HV, KV)                                                                        \
  if constexpr (HV == 128)                                                                      \
    hipLaunchKernelGGL((k_linear_dgrad_v5<HV, KV>), grid, block, lds, stream, a, tab, n16);     \
  else                                                                                          \
    hipLaunchKernelGGL((k_linear_dgrad_v4<HV, KV>), grid, block, lds, stream, a, tab, n16);
    HGNN_V4_SHAPES(HGNN_DG4)
#undef HGNN_DG4
    if (int rc = check_launch("k_linear_dgrad_v4")) return rc;
  }
  if (!wg) return HGNN_OK;
  if (!ws) return fail(HGNN_E_WS, "linear_bwd: weight gradients need the workspace");
  if (a.dz_out && !fused) {   // the dgrad kernel wrote the masked dz: wgrad streams it alone
    a.dout = a.dz_out;
    a.out_act = nullptr;
    a.mask_in = nullptr;
    a.dz_out = nullptr;
  }
  a.slab = static_cast<float*>(ws);
  const dim3 block(512);
  // wgrad v5 (every wave on MFMAs), 16-row tiles: H = K = 128 2.86 vs 4.73 ms (v4) at N = 9M;
  // v4 kept elsewhere (K = 256: v5 6.44 / 9.51 ms at T = 16 / 32 vs 5.65; H = 64 needs T >= 32,
  // which measured slower than v4: 2.44 vs 1.94 ms)
  constexpr int wg_t = 16;
  if (split) {
    const int64_t n_tiles = cdiv(a.n, wg_t);
    const size_t lds = wgrad5_lds(h, K, wg_t);
    const int64_t G = std::min<int64_t>(n_tiles, kBlocks * blocks_per_cu(lds));
    if (ws_bytes < slab_bytes(G, h, K)) return fail(HGNN_E_WS, "linear_bwd: workspace too small");
    *slabs = G;
    hipLaunchKernelGGL((k_linear_wgrad_v5<128, 128, wg_t>), dim3((unsigned)G), block, lds, stream,
                       a, tab, n_tiles);
    return check_launch("k_linear_wgrad_v5");
  }
  const int T = v4_bwd_lds(h, K, fused, 64) <= kLdsPerCu ? 64 : 32;
  const int64_t n_tiles = cdiv(a.n, T);
  const int64_t G = std::min<int64_t>(n_tiles, kBlocks);
  const size_t lds = v4_bwd_lds(h, K, fused, T);
  if (ws_bytes < slab_bytes(G, h, K)) return fail(HGNN_E_WS, "linear_bwd: workspace too small");
  *slabs = G;
  const dim3 grid((unsigned)G);
  // fused: K <= 128 (T = 64); wgrad-only: T = 32 at K = 256; H = K = 128 took wgrad v5 above
#define HGNN_BWD4L(HV, KV, DXV, TV) \
  hipLaunchKernelGGL((k_linear_bwd_v4<HV, KV, DXV, TV>), grid, block, lds, stream, a, tab, n_tiles)
#define HGNN_BWD4(HV, KV)                                         \
  if constexpr (!(HV == 128 && KV == 128)) {                      \
    if constexpr (KV <= 128) if (fused) HGNN_BWD4L(HV, KV, true, 64); \
    if (!fused) HGNN_BWD4L(HV, KV, false, (KV == 256 ? 32 : 64)); \
  }
  HGNN_V4_SHAPES(HGNN_BWD4)
#undef HGNN_BWD4
#undef HGNN_BWD4L
  return check_launch("k_linear_bwd_v4");
}

}  // namespace hgnn

