// Shared helpers for the hgnn HIP kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/hgnn.h"
#include "bce_terms.h"

namespace hgnn {

constexpr int kWave = 64;   // CDNA wavefront; never 32

// Thread-local last error (hgnn_last_error_string).
void set_error(const char* fmt, ...);

inline int fail(int code, const char* fmt, ...) {
  char buf[384];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  set_error("%s", buf);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HGNN_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return HGNN_OK;
}

inline hipStream_t as_stream(hgnn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// Bump allocator over the caller's workspace (the library owns no persistent memory).
struct Workspace {
  char* base;
  size_t cap;
  size_t used = 0;
  Workspace(void* p, size_t c) : base(static_cast<char*>(p)), cap(c) {}
  template <typename T>
  T* take(size_t n) {
    size_t off = align_up(used, 256);
    used = off + n * sizeof(T);
    return used <= cap && base ? reinterpret_cast<T*>(base + off) : nullptr;
  }
};

// Row fragments: W = 4 (float4 per lane) when d % 4 == 0, else scalar.
template <int W>
struct Vec;
template <>
struct Vec<4> {
  using T = float4;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T load(const float* p) {
    return *reinterpret_cast<const float4*>(p);
  }
  // streaming (nt) load: for rows gathered once per edge
  static __device__ __forceinline__ T load_nt(const float* p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  }
  static __device__ __forceinline__ void store(float* p, T v) {
    *reinterpret_cast<float4*>(p) = v;
  }
  static __device__ __forceinline__ void store_nt(float* p, T v) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(f4{v.x, v.y, v.z, v.w}, reinterpret_cast<f4*>(p));
  }
  static __device__ __forceinline__ void fma(T& a, float w, T v) {
    a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
  }
  static __device__ __forceinline__ void add(T& a, T v) {
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  static __device__ __forceinline__ float dot(T a, T b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
  }
  static __device__ __forceinline__ void scale(T& a, float s) {
    a.x *= s; a.y *= s; a.z *= s; a.w *= s;
  }
  static __device__ __forceinline__ T shfl_xor(T v, int m) {
    return make_float4(__shfl_xor(v.x, m, 64), __shfl_xor(v.y, m, 64), __shfl_xor(v.z, m, 64),
                       __shfl_xor(v.w, m, 64));
  }
};
template <>
struct Vec<1> {
  using T = float;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ T load_nt(const float* p) { return __builtin_nontemporal_load(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
  static __device__ __forceinline__ void store_nt(float* p, T v) { __builtin_nontemporal_store(v, p); }
  static __device__ __forceinline__ void fma(T& a, float w, T v) { a = fmaf(w, v, a); }
  static __device__ __forceinline__ void add(T& a, T v) { a += v; }
  static __device__ __forceinline__ float dot(T a, T b) { return a * b; }
  static __device__ __forceinline__ void scale(T& a, float s) { a *= s; }
  static __device__ __forceinline__ T shfl_xor(T v, int m) { return __shfl_xor(v, m, 64); }
};

// W = 8: the fragment of a bf16 source row (16 B = 8 elements per lane) widened to fp32; the
// fp32 side of such a gather (accumulators, output rows) is two float4 per lane.
struct float8 {
  float4 lo, hi;
};
template <>
struct Vec<8> {
  using T = float8;
  using H = Vec<4>;
  static __device__ __forceinline__ T zero() { return T{H::zero(), H::zero()}; }
  static __device__ __forceinline__ T load(const float* p) { return T{H::load(p), H::load(p + 4)}; }
  static __device__ __forceinline__ T load_nt(const float* p) {
    return T{H::load_nt(p), H::load_nt(p + 4)};
  }
  static __device__ __forceinline__ void store(float* p, T v) {
    H::store(p, v.lo);
    H::store(p + 4, v.hi);
  }
  static __device__ __forceinline__ void store_nt(float* p, T v) {
    H::store_nt(p, v.lo);
    H::store_nt(p + 4, v.hi);
  }
  static __device__ __forceinline__ void fma(T& a, float w, T v) {
    H::fma(a.lo, w, v.lo);
    H::fma(a.hi, w, v.hi);
  }
  static __device__ __forceinline__ void add(T& a, T v) {
    H::add(a.lo, v.lo);
    H::add(a.hi, v.hi);
  }
  static __device__ __forceinline__ float dot(T a, T b) {
    float s = H::dot(a.lo, b.lo);
    s = fmaf(a.hi.x, b.hi.x, s); s = fmaf(a.hi.y, b.hi.y, s);
    s = fmaf(a.hi.z, b.hi.z, s); s = fmaf(a.hi.w, b.hi.w, s);
    return s;
  }
  static __device__ __forceinline__ void scale(T& a, float s) {
    H::scale(a.lo, s);
    H::scale(a.hi, s);
  }
  static __device__ __forceinline__ T shfl_xor(T v, int m) {
    return T{H::shfl_xor(v.lo, m), H::shfl_xor(v.hi, m)};
  }
};

// The source rows of a gather, by element type.  fp32 rows (XT = float) are read as the fragment
// itself and `widen` is the identity, so those kernels are the code they were.  bf16 rows (XT =
// uint16_t, W = 8) are read 16 B per lane, stay packed (4 registers per vector) while in flight
// and are widened where they are summed: a shift or a mask per element, exact.
template <typename XT, int W>
struct RowSrc {
  using V = Vec<W>;
  using Raw = typename V::T;
  static __device__ __forceinline__ Raw zero() { return V::zero(); }
  static __device__ __forceinline__ Raw load(const float* p) { return V::load(p); }
  static __device__ __forceinline__ Raw load_nt(const float* p) { return V::load_nt(p); }
  static __device__ __forceinline__ typename V::T widen(Raw r) { return r; }
};
template <>
struct RowSrc<uint16_t, 8> {
  using Raw = uint4;
  static __device__ __forceinline__ Raw zero() { return make_uint4(0u, 0u, 0u, 0u); }
  static __device__ __forceinline__ Raw load(const uint16_t* p) {
    return *reinterpret_cast<const uint4*>(p);
  }
  static __device__ __forceinline__ Raw load_nt(const uint16_t* p) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const u4 v = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  // element 2k sits in the low half of word k, element 2k + 1 in its high half
  static __device__ __forceinline__ float4 widen2(uint32_t a, uint32_t b) {
    return make_float4(__uint_as_float(a << 16), __uint_as_float(a & 0xffff0000u),
                       __uint_as_float(b << 16), __uint_as_float(b & 0xffff0000u));
  }
  static __device__ __forceinline__ float8 widen(Raw r) {
    return float8{widen2(r.x, r.y), widen2(r.z, r.w)};
  }
};

// Device exclusive scan of int32 counts (n entries) -> out (n+1 entries, out[n] = total).
// Workspace query with ws == nullptr.
// Sum over aligned groups of LPR lanes (power of 2), result in every lane of the group.  Within a
// 16-lane DPP row the butterfly runs on DPP moves (quad_perm xor 1 / xor 2, row_half_mirror,
// row_mirror) instead of LDS-pipe ds_bpermute; wider groups finish with shuffles.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}
template <int LPR>
__device__ __forceinline__ float slot_sum(float s) {
  if constexpr (LPR >= 2) s += dpp_mov<0xB1>(s);    // quad_perm [1,0,3,2]
  if constexpr (LPR >= 4) s += dpp_mov<0x4E>(s);    // quad_perm [2,3,0,1]
  if constexpr (LPR >= 8) s += dpp_mov<0x141>(s);   // row_half_mirror
  if constexpr (LPR >= 16) s += dpp_mov<0x140>(s);  // row_mirror
  if constexpr (LPR >= 32) s += __shfl_xor(s, 16, 64);
  if constexpr (LPR >= 64) s += __shfl_xor(s, 32, 64);
  return s;
}

// <a, b> over a slot's LPR lanes, each holding VPL fragments of W columns (the link loss's scoring
// kernels, scoring.hip, and the hard-negative miner, hardneg.hip)
template <int LPR, int VPL, int W>
__device__ __forceinline__ float slot_dot(const typename Vec<W>::T (&a)[VPL],
                                          const typename Vec<W>::T (&b)[VPL]) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < VPL; ++q) {
    if constexpr (W == 8) {
      s = fmaf(a[q].lo.x, b[q].lo.x, s); s = fmaf(a[q].lo.y, b[q].lo.y, s);
      s = fmaf(a[q].lo.z, b[q].lo.z, s); s = fmaf(a[q].lo.w, b[q].lo.w, s);
      s = fmaf(a[q].hi.x, b[q].hi.x, s); s = fmaf(a[q].hi.y, b[q].hi.y, s);
      s = fmaf(a[q].hi.z, b[q].hi.z, s); s = fmaf(a[q].hi.w, b[q].hi.w, s);
    } else if constexpr (W == 4) {
      s = fmaf(a[q].x, b[q].x, s); s = fmaf(a[q].y, b[q].y, s);
      s = fmaf(a[q].z, b[q].z, s); s = fmaf(a[q].w, b[q].w, s);
    } else {
      s = fmaf(a[q], b[q], s);
    }
  }
  return slot_sum<LPR>(s);
}

// (The BCE link loss's terms from t = exp(-|x|) -- exp_neg_abs, sigmoid_t, pos_coef_t, softplus_t
// -- are bce_terms.h's, included above: plain C++ that the host check compiles too.)

// Uniform int32 in [0, hi) of draw i: splitmix64 of seed + i * golden ratio, then the high 32 bits
// scaled by hi (hgnn_uniform_i32; the negatives sort regenerates the same draws in its first pass).
__device__ __forceinline__ int32_t uniform_draw(uint64_t seed, int64_t i, uint32_t hi) {
  uint64_t x = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (int32_t)(((x >> 32) * (uint64_t)hi) >> 32);
}

int exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t* ws_bytes,
                       hipStream_t stream);


}  // namespace hgnn
