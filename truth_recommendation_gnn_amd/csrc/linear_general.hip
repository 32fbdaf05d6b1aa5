// K3/K4 on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 fma chain) for any shape: the general
// forward / dgrad / wgrad kernels and the backward's LDS fast path, with their launchers.
// (linear.hip: what K3 computes, and which family a call takes.)
//
// MFMA operand trick: for a 16-wide K chunk, lane (i = lane&15, g = lane>>4) loads the float4
// X[row i][kc+4g .. kc+4g+3] and uses element q as the A operand of k-step q; B takes the same
// k from W.  So k-step q sums k = kc+4g+q over g — every k of the chunk exactly once, with
// contiguous 16-B loads (the k order inside a chunk is permuted, which only moves rounding).
#include "linear_common.h"

#include <algorithm>

namespace hgnn {

template <bool VEC>
__device__ __forceinline__ void load4(const float* p, int valid_elems, float (&v)[4]) {
  if (VEC) {
    if (valid_elems >= 4) {
      float4 t = *reinterpret_cast<const float4*>(p);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = q < valid_elems ? p[q] : 0.f;
  }
}

constexpr int RT = 2;             // 16-row tiles per wave
constexpr int kRowsPerBlock = 4 * RT * 16;

// ---------------------------------------------------------------- forward
template <int NT, bool VEC>
__global__ void __launch_bounds__(256) k_linear_fwd(const LinArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock + wave * (RT * 16);
  const int c0 = blockIdx.y * (NT * 16);
  f32x4 acc[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < a.n_seg; ++s) {
    const Seg sg = a.seg[s];
    for (int kc = 0; kc < sg.k; kc += 16) {
      const int k = kc + 4 * g;
      const int kv = sg.k - k;  // valid elements from k
      float av[RT][4], bv[NT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int64_t row = r0 + rt * 16 + i;
        if (row < a.n) load4<VEC>(sg.x + row * sg.k + k, kv, av[rt]);
        else av[rt][0] = av[rt][1] = av[rt][2] = av[rt][3] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = c0 + t * 16 + i;
        if (col < a.h) load4<VEC>(a.w + (int64_t)col * a.k_total + sg.off + k, kv, bv[t]);
        else bv[t][0] = bv[t][1] = bv[t][2] = bv[t][3] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[rt][t] = mfma4(av[rt][q], bv[t][q], acc[rt][t]);
    }
  }
  // C/D map of 16x16x4: col = lane&15, row = 4*(lane>>4) + reg
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = c0 + t * 16 + i;
    if (col >= a.h) continue;
    const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t row = r0 + rt * 16 + 4 * g + j;
        if (row < a.n) {
          float v = acc[rt][t][j] + b;
          if (a.relu) v = fmaxf(v, 0.f);
          a.out[row * a.h + col] = v;
        }
      }
  }
}

// ---------------------------------------------------------------- dgrad: dX_s = dZ @ W_s
template <bool VEC>
__device__ __forceinline__ void load_dz(const LinArgs& a, int64_t row, int j, float (&v)[4]) {
  const int jv = a.h - j;
  if (row >= a.n) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
  load4<VEC>(a.dout + row * a.h + j, jv, v);
  if (a.out_act) {
    float m[4];
    load4<VEC>(a.out_act + row * a.h + j, jv, m);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = m[q] > 0.f ? v[q] : 0.f;
  }
}

template <int NT, bool VEC>
__global__ void __launch_bounds__(256) k_linear_dgrad(const LinArgs a) {
  const int c0 = blockIdx.y * (NT * 16);
  bool any = false;
  for (int s = 0; s < a.n_seg; ++s)
    any |= a.seg[s].dx && a.seg[s].off < c0 + NT * 16 && a.seg[s].off + a.seg[s].k > c0;
  if (!any) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock + wave * (RT * 16);
  f32x4 acc[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int jc = 0; jc < a.h; jc += 16) {
    const int j = jc + 4 * g;
    float av[RT][4], bv[NT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) load_dz<VEC>(a, r0 + rt * 16 + i, j, av[rt]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = c0 + t * 16 + i;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        bv[t][q] = (col < a.k_total && j + q < a.h) ? a.w[(int64_t)(j + q) * a.k_total + col]
                                                    : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = mfma4(av[rt][q], bv[t][q], acc[rt][t]);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = c0 + t * 16 + i;
    if (col >= a.k_total) continue;
    int s = 0;
    while (s + 1 < a.n_seg && col >= a.seg[s].off + a.seg[s].k) ++s;
    float* dx = a.seg[s].dx;
    if (!dx) continue;
    const int kk = col - a.seg[s].off, ks = a.seg[s].k;
    const bool add = (a.dx_acc >> s) & 1u;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int64_t row = r0 + rt * 16 + 4 * g + jj;
        if (row < a.n) {
          float* p = dx + row * ks + kk;
          *p = add ? *p + acc[rt][t][jj] : acc[rt][t][jj];
        }
      }
  }
}

// ---------------------------------------------------------------- wgrad partials
// Block: 4 waves, j range of 64 (blockIdx.z), k range of 128 over [X_0..X_{S-1}, 1] (blockIdx.y;
// the trailing ones column gives db), rows [bx*rows_per_block, ...) staged 32 at a time in LDS.
constexpr int WG_ROWS = 32;
constexpr int WG_J = 64;
constexpr int WG_K = 128;
constexpr int DZ_LD = WG_J + 16;   // row stride = 16 mod 32 banks: lanes g and g+1 disjoint
constexpr int X_LD = WG_K + 16;

template <bool VEC>
__global__ void __launch_bounds__(256) k_linear_wgrad(const LinArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[WG_ROWS * DZ_LD + WG_ROWS * X_LD];
  float* dz_l = lds;
  float* x_l = lds + WG_ROWS * DZ_LD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.z * WG_J, k0 = blockIdx.y * WG_K;
  const int kext = a.k_total + 1;
  const int64_t rb = (int64_t)blockIdx.x * a.rows_per_block;
  const int64_t re = min<int64_t>(rb + a.rows_per_block, a.n);
  f32x4 acc[WG_K / 16];
#pragma unroll
  for (int t = 0; t < WG_K / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t rs = rb; rs < re; rs += WG_ROWS) {
    // stage dZ[32][64] (masked) and X[32][128]: one float4 per (row, 4 columns)
    for (int idx = threadIdx.x; idx < WG_ROWS * (WG_J / 4); idx += 256) {
      const int r = idx / (WG_J / 4), c4 = idx % (WG_J / 4);
      float v[4];
      load_dz<VEC>(a, rs + r < re ? rs + r : a.n, j0 + 4 * c4, v);
      *reinterpret_cast<float4*>(dz_l + r * DZ_LD + 4 * c4) = make_float4(v[0], v[1], v[2], v[3]);
    }
    for (int idx = threadIdx.x; idx < WG_ROWS * (WG_K / 4); idx += 256) {
      const int r = idx / (WG_K / 4), c4 = idx % (WG_K / 4);
      const int64_t row = rs + r;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (row < re) {
        const int kg = k0 + 4 * c4;
        if (VEC && kg + 4 <= a.k_total) {
          int s = 0;
          while (s + 1 < a.n_seg && kg >= a.seg[s].off + a.seg[s].k) ++s;
          const float4 t =
              *reinterpret_cast<const float4*>(a.seg[s].x + row * a.seg[s].k + kg - a.seg[s].off);
          v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int kq = kg + q;
            if (kq < a.k_total) {
              int s = 0;
              while (s + 1 < a.n_seg && kq >= a.seg[s].off + a.seg[s].k) ++s;
              v[q] = a.seg[s].x[row * a.seg[s].k + kq - a.seg[s].off];
            } else if (kq == a.k_total) {
              v[q] = 1.f;
            }
          }
        }
      }
      *reinterpret_cast<float4*>(x_l + r * X_LD + 4 * c4) = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    // A[i = j][kk = row] = dZ[row][j], B[kk = row][col = k] = X[row][k]; k-step s covers rows 4s..4s+3
#pragma unroll
    for (int s = 0; s < WG_ROWS / 4; ++s) {
      const int r = 4 * s + g;
      const float av = dz_l[r * DZ_LD + wave * 16 + i];
#pragma unroll
      for (int t = 0; t < WG_K / 16; ++t) acc[t] = mfma4(av, x_l[r * X_LD + t * 16 + i], acc[t]);
    }
    __syncthreads();
  }
  // partial tile: rows j = j0 + wave*16 + 4g + jj, cols k = k0 + 16t + i
  float* slab = a.slab + (int64_t)blockIdx.x * a.h * kext;
#pragma unroll
  for (int t = 0; t < WG_K / 16; ++t) {
    const int k = k0 + t * 16 + i;
    if (k >= kext) continue;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = j0 + wave * 16 + 4 * g + jj;
      if (j < a.h) slab[(int64_t)j * kext + k] = acc[t][jj];
    }
  }
}

// ================================================================ fused backward (LDS path)
// When W fits in LDS (h*K*4 <= 64 KiB), h % 16 == 0, K % 32 == 0 and every segment is float4-
// aligned: persistent blocks keep W^T resident in LDS and stream 32-row tiles of dz and X
// through LDS once (register prefetch of the next tile overlaps HBM with the MFMAs), computing
// dX and the block's dW/db from the same staged tiles.  (An LDS-staged forward built the same
// way measured no faster than the direct-fragment forward — 345 vs 325 us at N=1M, K=128, h=64,
// both MFMA-issue bound at ~50 TF/s — so the forward keeps the direct kernel.)
constexpr int FT = 32;  // rows per tile

// Register prefetch of one [FT x K] tile (K <= 128 => at most 4 float4 per thread): issued
// before the current tile's MFMAs so HBM latency overlaps compute, stored to LDS after.
struct XPrefetch {
  float4 v[4];
  __device__ __forceinline__ void load(const LinArgs& a, int64_t r0) {
    const int k4 = a.k_total >> 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = threadIdx.x + 256 * q;
      v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < FT * k4) {
        const int r = idx / k4, k = (idx - r * k4) * 4;
        int s = 0;
        while (s + 1 < a.n_seg && k >= a.seg[s].off + a.seg[s].k) ++s;
        const int64_t row = r0 + r;
        if (row < a.n)
          v[q] = *reinterpret_cast<const float4*>(a.seg[s].x + row * a.seg[s].k +
                                                  (k - a.seg[s].off));
      }
    }
  }
  __device__ __forceinline__ void store(const LinArgs& a, float* xs, int ld) const {
    const int k4 = a.k_total >> 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = threadIdx.x + 256 * q;
      if (idx < FT * k4) {
        const int r = idx / k4, k = (idx - r * k4) * 4;
        *reinterpret_cast<float4*>(xs + r * ld + k) = v[q];
      }
    }
  }
};

// Fused backward: per 32-row tile, dz = dout * (out > 0) and X staged once; dX = dz @ W (W^T in
// LDS) and the block's dW (+ db as the column K) accumulated in registers across its tiles,
// written once as a partial [h][K+1] slab (reduced in block order by k_wgrad_reduce).
template <int NT, bool DX>
__global__ void __launch_bounds__(256) k_linear_bwd_lds(const LinArgs a, int64_t n_tiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.k_total, h = a.h;
  const int ldwt = h + 4, ldz = h + 16, ldx = K + 16;   // b32 reads: row stride = 16 mod 32
  float* wt = smem;                 // [K][ldwt]  W^T
  float* dz = wt + K * ldwt;        // [FT][ldz]
  float* xs = dz + FT * ldz;        // [FT][ldx]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  constexpr int JT = NT >= 4 ? NT / 4 : 1;      // j tiles per wave (wgrad)
  const bool wave_has_j = NT >= 4 || wave < NT;
  const int KT = K >> 4;
  if (DX) {
    for (int idx = threadIdx.x; idx < h * K; idx += 256) {
      const int j = idx / K, k = idx - j * K;
      wt[k * ldwt + j] = a.w[(int64_t)j * K + k];
    }
  }
  f32x4 acc[JT][8];   // K <= 128 on this path
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) acc[jt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int h4 = h >> 2;
  // prefetch registers: dz (dout masked by out) <= 4 float4, X <= 4 float4 per thread
  float4 zp[4];
  XPrefetch pf;
  auto load_dz = [&](int64_t r0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = threadIdx.x + 256 * q;
      zp[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < FT * h4) {
        const int r = idx / h4, c = (idx - r * h4) * 4;
        const int64_t row = r0 + r;
        if (row < a.n) {
          float4 v = *reinterpret_cast<const float4*>(a.dout + row * h + c);
          if (a.out_act) {
            const float4 m = *reinterpret_cast<const float4*>(a.out_act + row * h + c);
            v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
            v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
          }
          zp[q] = v;
        }
      }
    }
  };
  load_dz((int64_t)blockIdx.x * FT);
  pf.load(a, (int64_t)blockIdx.x * FT);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * FT;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = threadIdx.x + 256 * q;
      if (idx < FT * h4) {
        const int r = idx / h4, c = (idx - r * h4) * 4;
        const float4 v = zp[q];
        dbacc.x += v.x; dbacc.y += v.y; dbacc.z += v.z; dbacc.w += v.w;
        *reinterpret_cast<float4*>(dz + r * ldz + c) = v;
      }
    }
    pf.store(a, xs, ldx);
    __syncthreads();
    if (tile + gridDim.x < n_tiles) {
      load_dz((tile + gridDim.x) * FT);
      pf.load(a, (tile + gridDim.x) * FT);
    }
    if (DX) {   // dX tile [FT x K]: wave = row tile (wave & 1) x column half (wave >> 1)
      const int rt = wave & 1, half = wave >> 1;
      const int ct0 = half * (KT >> 1), nct = KT >> 1;
      for (int c = 0; c < nct; ++c) {
        const int ct = ct0 + c;
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int jc = 0; jc < h; jc += 16) {
          const float4 av = *reinterpret_cast<const float4*>(dz + (rt * 16 + i) * ldz + jc + 4 * g);
          const float4 bv = *reinterpret_cast<const float4*>(wt + (ct * 16 + i) * ldwt + jc + 4 * g);
          o = mfma4(av.x, bv.x, o);
          o = mfma4(av.y, bv.y, o);
          o = mfma4(av.z, bv.z, o);
          o = mfma4(av.w, bv.w, o);
        }
        const int col = ct * 16 + i;
        int s = 0;
        while (s + 1 < a.n_seg && col >= a.seg[s].off + a.seg[s].k) ++s;
        float* dx = a.seg[s].dx;
        if (dx) {
          const int kk = col - a.seg[s].off, ks = a.seg[s].k;
          const bool add = (a.dx_acc >> s) & 1u;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t row = r0 + rt * 16 + 4 * g + r;
            if (row < a.n) {
              float* p = dx + row * ks + kk;
              *p = add ? *p + o[r] : o[r];
            }
          }
        }
      }
    }
    if (wave_has_j) {   // wgrad: A[i=j][kk=row] = dz[row][j], B[kk=row][col=k] = X[row][k]
#pragma unroll 2
      for (int s4 = 0; s4 < FT / 4; ++s4) {
        const int r = 4 * s4 + g;
        float bv[8];
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) bv[kt] = kt < KT ? xs[r * ldx + kt * 16 + i] : 0.f;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
          const float av = dz[r * ldz + (wave + 4 * jt) * 16 + i];
#pragma unroll
          for (int kt = 0; kt < 8; ++kt)
            if (kt < KT) acc[jt][kt] = mfma4(av, bv[kt], acc[jt][kt]);
        }
      }
    }
  }
  // partial slab [blockIdx.x][h][K+1]
  const int kext = K + 1;
  float* slab = a.slab + (int64_t)blockIdx.x * h * kext;
  if (wave_has_j) {
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        if (kt >= KT) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = (wave + 4 * jt) * 16 + 4 * g + r;
          slab[(int64_t)j * kext + kt * 16 + i] = acc[jt][kt][r];
        }
      }
  }
  __syncthreads();
  float4* red = reinterpret_cast<float4*>(xs);     // [256] thread partials of db
  red[threadIdx.x] = dbacc;
  __syncthreads();
  if (threadIdx.x < h4) {   // thread t staged columns 4*(t % h4) on every tile
    float4 t = red[threadIdx.x];
    for (int m = threadIdx.x + h4; m < 256; m += h4) {
      const float4 u = red[m];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    const int c = threadIdx.x * 4;
    slab[(int64_t)(c + 0) * kext + K] = t.x;
    slab[(int64_t)(c + 1) * kext + K] = t.y;
    slab[(int64_t)(c + 2) * kext + K] = t.z;
    slab[(int64_t)(c + 3) * kext + K] = t.w;
  }
}

// ================================================================ launchers
// KERN<NT, vec> on a (gx, gy) grid
#define HGNN_GEN(KERN, NT, GX, GY)                                                               \
  do {                                                                                           \
    const dim3 grid((unsigned)(GX), (unsigned)(GY));                                             \
    if (vec) hipLaunchKernelGGL((KERN<NT, true>), grid, dim3(256), 0, stream, a);                \
    else hipLaunchKernelGGL((KERN<NT, false>), grid, dim3(256), 0, stream, a);                   \
  } while (0)

int gen_linear_fwd(const LinArgs& a, bool vec, hipStream_t stream) {
  const unsigned gx = (unsigned)cdiv(a.n, kRowsPerBlock);
  // few row blocks (a sampled block's 2k-32k destination rows at K = 384): 32-column tiles give
  // 4x the workgroups (measured 47 us for 2048 rows on 16 workgroups of 128 columns)
  if ((int64_t)gx * cdiv(a.h, 128) < 1024) HGNN_GEN(k_linear_fwd, 2, gx, cdiv(a.h, 32));
  else if (a.h <= 64) HGNN_GEN(k_linear_fwd, 4, gx, 1);
  else HGNN_GEN(k_linear_fwd, 8, gx, cdiv(a.h, 128));
  return check_launch("k_linear_fwd");
}

// the wgrad's row blocks (its slabs) and *rpb rows in each
static int64_t wgrad_grid(int64_t n_rows, int32_t k_total, int32_t h, int64_t* rpb) {
  const int64_t gy = cdiv(k_total + 1, WG_K), gz = cdiv(h, WG_J);
  const int64_t tiles = cdiv(n_rows, WG_ROWS);
  int64_t want = std::max<int64_t>(1, 1024 / (gy * gz));
  const int64_t cap = std::max<int64_t>(1, (int64_t(64) << 20) / ((int64_t)h * (k_total + 1) * 4));
  want = std::min(want, cap);
  want = std::max<int64_t>(1, std::min(want, tiles));
  *rpb = cdiv(tiles, want) * WG_ROWS;
  return std::max<int64_t>(1, cdiv(n_rows, *rpb));
}

int64_t gen_bwd_slabs(int64_t n_rows, int32_t k_total, int32_t h) {
  int64_t rpb;
  return wgrad_grid(n_rows, k_total, h, &rpb);
}

int gen_linear_bwd(LinArgs a, bool vec, bool dx, bool wg, void* ws, size_t ws_bytes,
                   int64_t* slabs, hipStream_t stream) {
  if (dx) {
    const int64_t gxd = cdiv(a.n, kRowsPerBlock);
    // few row blocks: 32-column tiles (see forward)
    if (gxd * cdiv(a.k_total, 128) < 1024) HGNN_GEN(k_linear_dgrad, 2, gxd, cdiv(a.k_total, 32));
    else HGNN_GEN(k_linear_dgrad, 8, gxd, cdiv(a.k_total, 128));
    if (int rc = check_launch("k_linear_dgrad")) return rc;
  }
  if (!wg) return HGNN_OK;
  int64_t rpb;
  const int64_t gx = wgrad_grid(a.n, a.k_total, a.h, &rpb);
  if (!ws || ws_bytes < slab_bytes(gx, a.h, a.k_total))
    return fail(HGNN_E_WS, "linear_bwd: workspace too small");
  a.slab = static_cast<float*>(ws);
  a.rows_per_block = rpb;
  *slabs = gx;
  const dim3 grid((unsigned)gx, (unsigned)cdiv(a.k_total + 1, WG_K), (unsigned)cdiv(a.h, WG_J));
  if (vec) hipLaunchKernelGGL(k_linear_wgrad<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(k_linear_wgrad<false>, grid, dim3(256), 0, stream, a);
  return check_launch("k_linear_wgrad");
}
#undef HGNN_GEN

bool lds_bwd_ok(const LinArgs& a, bool vec) {
  return vec && a.h % 16 == 0 && a.h <= 128 && a.k_total % 32 == 0 && a.k_total <= 128 &&
         (size_t)a.h * a.k_total * 4 <= 65536 && 256 % (a.h / 4) == 0;
}

int64_t lds_bwd_slabs(int64_t n_rows) {
  return std::max<int64_t>(1, std::min<int64_t>(cdiv(n_rows, FT), 512));
}

int lds_linear_bwd(LinArgs a, bool dx, void* ws, size_t ws_bytes, int64_t* slabs,
                   hipStream_t stream) {
  const int64_t n_tiles = cdiv(a.n, FT);
  const int64_t G = lds_bwd_slabs(a.n);
  if (!ws || ws_bytes < slab_bytes(G, a.h, a.k_total))
    return fail(HGNN_E_WS, "linear_bwd: workspace too small");
  a.slab = static_cast<float*>(ws);
  *slabs = G;
  const size_t lds = ((size_t)a.k_total * (a.h + 4) + (size_t)FT * (a.h + 16) +
                      (size_t)FT * (a.k_total + 16)) * 4;
  const dim3 grid((unsigned)G), block(256);
#define HGNN_BWD_LDS(NTV)                                                                      \
  if (dx) hipLaunchKernelGGL((k_linear_bwd_lds<NTV, true>), grid, block, lds, stream, a,       \
                             n_tiles);                                                         \
  else hipLaunchKernelGGL((k_linear_bwd_lds<NTV, false>), grid, block, lds, stream, a, n_tiles);
  switch (a.h / 16) {
    case 1: HGNN_BWD_LDS(1) break;
    case 2: HGNN_BWD_LDS(2) break;
    case 4: HGNN_BWD_LDS(4) break;
    case 8: HGNN_BWD_LDS(8) break;
    default: return fail(HGNN_E_UNSUPPORTED, "linear_bwd fast path: h=%d", a.h);
  }
#undef HGNN_BWD_LDS
  return check_launch("k_linear_bwd_lds");
}

}  // namespace hgnn
