// K3/K4: fused multi-segment linear on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 fma chain).
//
//   out[n, h] = act( sum_s X_s[n, K_s] @ W[:, off_s : off_s+K_s]^T + b )
//
// One call is a whole SAGE destination update: the segments are the per-relation mean
// aggregates and the destination's own features, W is the K-concatenation of the relation
// weights pre-scaled by the reference's fixed relation weights (train_gnn.py:163-164,187-198),
// act = ReLU.  That fuses lin_l + lin_r + weighted sum + bias + ReLU into one pass over HBM.
//
// The host side of every hgnn_linear_* call: the argument check (prepare_*), the
// choice of kernel family (*_path), the launch compositions (run_*), the slab reduce, the C ABI.
// The kernels and their launchers: linear_general.hip, linear_v4.hip, linear_xs.hip.
#include "linear_common.h"

#include <algorithm>
#include <stdlib.h>
#include <vector>

namespace hgnn {

// dw[j][k] = sum_b slab[b][j][k] (k < K), db[j] = sum_b slab[b][j][K]; fixed b order.
// ldd: dw's row stride (kext - 1, or the whole dW's K for a column block of it)
__device__ __forceinline__ void wgrad_reduce_body(const float* slab, int64_t nb, int32_t h,
                                                  int32_t kext, float* dw, float* db, int32_t ldd,
                                                  int64_t bid) {
  // 64 outputs per block (lanes), 16 waves each sum a contiguous range of slabs with 4
  // independent accumulators, then wave 0 adds the 16 partials in order: a fixed summation
  // order for a given nb (deterministic), and enough loads in flight to stream the slabs
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t e = bid * 64 + lane;
  const int64_t total = (int64_t)h * kext;
  const int64_t per = cdiv(nb, 16);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < total) {
    const int64_t b1 = min<int64_t>((wave + 1) * per, nb);
    int64_t b = wave * per;
    for (; b + 4 <= b1; b += 4) {
      s0 += slab[b * total + e];
      s1 += slab[(b + 1) * total + e];
      s2 += slab[(b + 2) * total + e];
      s3 += slab[(b + 3) * total + e];
    }
    for (; b < b1; ++b) s0 += slab[b * total + e];
  }
  part[wave][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wave == 0 && e < total) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) v += part[w][lane];
    const int j = (int)(e / kext), k = (int)(e % kext);
    if (k < kext - 1) { if (dw) dw[(int64_t)j * ldd + k] = v; }
    else if (db) db[j] = v;
  }
}

__global__ void __launch_bounds__(1024) k_wgrad_reduce(const float* slab, int64_t nb, int32_t h,
                                                       int32_t kext, float* dw, float* db,
                                                       int32_t ldd) {
  wgrad_reduce_body(slab, nb, h, kext, dw, db, ldd, blockIdx.x);
}

// Two jobs' slabs (the split kernels' two-job backward) in one launch: blocks [0, nblk0) reduce
// job 0, the rest job 1.  Each output is a fixed-order sum over its job's nb slabs: deterministic,
// but bitwise the job's own launch only while the pair keeps the job's own grid — once pair_grids
// rescales the grids, nb and the rows behind each partial sum differ (same sums, other rounding).
struct ReducePair {
  const float* slab[2];
  int64_t nb[2];
  float* dw[2];
  float* db[2];
  int64_t nblk0;
  int32_t h, kext, ldd;
};
__global__ void __launch_bounds__(1024) k_wgrad_reduce2(const ReducePair p) {
  if ((int64_t)blockIdx.x < p.nblk0)
    wgrad_reduce_body(p.slab[0], p.nb[0], p.h, p.kext, p.dw[0], p.db[0], p.ldd, blockIdx.x);
  else
    wgrad_reduce_body(p.slab[1], p.nb[1], p.h, p.kext, p.dw[1], p.db[1], p.ldd,
                      (int64_t)blockIdx.x - p.nblk0);
}

// The bf16x6 K3 kernels (H = 128, K = 128 / 256): on unless HGNN_K3_X6=0, or as last set by
// hgnn_set_k3_split (tests run both paths in one process).
static int g_k3_x6 = -1;
static bool x6_enabled() {
  if (g_k3_x6 < 0) g_k3_x6 = (!getenv("HGNN_K3_X6") || atoi(getenv("HGNN_K3_X6")) != 0) ? 1 : 0;
  return g_k3_x6 != 0;
}

// ReLU mask bits from a finished output (forward shapes without a persistent kernel), in the
// lane layout of mask4: one thread per (row, lane group g).
__global__ void k_relu_mask(const float* out, int64_t n, int32_t h, uint32_t* mask) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * 4) return;
  const int64_t row = idx >> 2;
  const int g = (int)(idx & 3);
  uint32_t m = 0;
  for (int c = 0; c < h / 16; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      m |= (out[row * h + 16 * c + 4 * g + e] > 0.f ? 1u : 0u) << (4 * c + e);
  mask[idx] = m;
}

// dw / db from the nb slabs [h][K + 1] a backward launcher left in the workspace, in block order
static int reduce_slab(const void* slab, int64_t nb, int32_t h, int32_t K, float* dw, float* db,
                       hipStream_t stream) {
  const int64_t total = (int64_t)h * (K + 1);
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)cdiv(total, 64)), dim3(1024), 0, stream,
                     static_cast<const float*>(slab), nb, h, K + 1, dw, db, K);
  return check_launch("k_wgrad_reduce");
}

// ================================================================ shapes
// the persistent kernels' shapes: v4 / v5, and the split at H = 128, K = 128 / 256
static bool v4_ok(const LinArgs& a, bool vec) {
  if (!vec || !(a.h == 64 || a.h == 128) ||
      !(a.k_total == 64 || a.k_total == 128 || a.k_total == 256))
    return false;
  for (int s = 0; s < a.n_seg; ++s)
    if (a.seg[s].k % 16) return false;
  return true;
}

// the fp32-exact bf16x6 split at H = 128, K = 128 / 256 (linear_xs.hip), the default
// (hgnn_set_k3_split(0) / HGNN_K3_X6=0: the f32-input v4 / v5 kernels, the one fallback)
static bool split_shape(const LinArgs& a) {
  return x6_enabled() && a.h == 128 && (a.k_total == 128 || a.k_total == 256);
}

// the chunks of columns [c0, c0 + kp) of the concatenated input (every segment a multiple of 16)
static ChunkTab chunk_table_range(const LinArgs& a, int c0, int kp) {
  ChunkTab t{};
  for (int c = 0; c < kp / 16 && c < kMaxChunks; ++c) {
    const int k = c0 + c * 16;
    int s = 0;
    while (s + 1 < a.n_seg && k >= a.seg[s].off + a.seg[s].k) ++s;
    t.x[c] = a.seg[s].x;
    t.dx[c] = a.seg[s].dx;
    if ((a.dx_acc >> s) & 1u) t.dx_acc |= 1u << c;
    t.ld[c] = a.seg[s].k;
    t.col[c] = k - a.seg[s].off;
  }
  return t;
}
static ChunkTab chunk_table(const LinArgs& a) { return chunk_table_range(a, 0, a.k_total); }

// K = 384 / 512 at H = 128 (the sampled blocks' [aggr_1 | aggr_2 | root] at d = 128) on the
// split-once kernels as two column blocks, [0, 256) and [256, K): the forward's second launch
// adds the first one's output rows (its own `add`, read before the same block stores them)
// and applies the bias, activation and mask; the backward runs each block's dgrad / wgrad into
// its columns of one shared [G][h][K + 1] slab, reduced once.  Replaces the f32-input general
// kernels there (51 / 65 us per launch at cfg5's ~17k rows).
// Blocks of every size take it: at cfg5's inner blocks (2-3k rows) the general kernels measured
// the same time one destination type at a time (0.680 vs 0.677 ms per batch, 4 launches fewer),
// but with both types paired into one launch per column block (hgnn_linear_fwd_multi) the split
// kernels are faster: 0.603 / 0.604 vs 0.622 / 0.621 ms per batch, 22 vs 24 launches
// (profiles/r6_wide_min_ab.txt).
static bool xs_wide_ok(const LinArgs& a, bool vec) {
  if (!vec || a.h != 128 || a.k_total <= 256 || a.k_total > 512 || a.k_total % 128 != 0)
    return false;
  for (int s = 0; s < a.n_seg; ++s)
    if (a.seg[s].k % 16) return false;
  return x6_enabled();
}

// The two column blocks pass the first one's partial rows through `out`, so out must not alias
// an input segment (or `add`) on this path; such a call goes to the general kernels instead
// (ADVICE r5).  Byte ranges of n rows each.
static bool out_overlaps_inputs(const LinArgs& a) {
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(a.out);
  const uintptr_t o1 = o0 + (uintptr_t)a.n * a.h * 4;
  auto hit = [&](const void* p, int64_t row_floats) {
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), p1 = p0 + (uintptr_t)a.n * row_floats * 4;
    return p && p0 < o1 && o0 < p1;
  };
  for (int s = 0; s < a.n_seg; ++s)
    if (hit(a.seg[s].x, a.seg[s].k)) return true;
  return hit(a.add, a.h);
}

// Column block `part`, [0, 256) or [256, K), of a K = 384 / 512 call.  Forward: block 0 leaves
// its partial rows (plus the caller's `add`) in out, block 1 adds them and applies bias, activation
// and mask.  Backward: the block's dX, and its dW columns at c0 of the call's one slab.
struct ColBlock {
  LinArgs a;
  ChunkTab tab;
  bool dx;   // backward: the block has a segment whose dX is wanted
};
static ColBlock column_block(const LinArgs& a, int part) {
  const int c0 = part ? 256 : 0, kp = part ? a.k_total - 256 : 256;
  ColBlock b{a, chunk_table_range(a, c0, kp), false};
  b.a.k_total = kp;
  b.a.w = a.w + c0;
  if (part == 0) {
    b.a.bias = nullptr;
    b.a.relu = 0;
    b.a.mask_out = nullptr;
  } else {
    b.a.add = a.out;
  }
  b.a.dz_out = nullptr;
  b.a.slab_ld = a.k_total + 1;
  b.a.slab_c0 = c0;
  for (int c = 0; c < kp / 16; ++c) b.dx |= b.tab.dx[c] != nullptr;
  return b;
}

// the split kernels' slab of a job, whole K (one slab for both column blocks)
static size_t split_slab_bytes(const LinArgs& a) {
  return slab_bytes(xs_bwd_grid(a.n), a.h, a.k_total);
}

// ================================================================ one prepared call per direction
static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// segments, W and the sizes; *vec: h, every segment width and base, and W allow float4 rows
static int fill_args(LinArgs& a, int32_t n_seg, const float* const* xs, const int32_t* ks,
                     float* const* dxs, int64_t n_rows, const float* w, int32_t h, bool* vec) {
  if (n_seg < 1 || n_seg > HGNN_MAX_SEG) return fail(HGNN_E_ARG, "linear: n_seg=%d", n_seg);
  if (h < 1 || n_rows < 0 || !w || !xs || !ks) return fail(HGNN_E_ARG, "linear: bad arguments");
  a.n_seg = n_seg;
  a.k_total = 0;
  *vec = (h % 4 == 0);
  for (int s = 0; s < n_seg; ++s) {
    if (ks[s] < 1 || (n_rows > 0 && !xs[s])) return fail(HGNN_E_ARG, "linear: segment %d", s);
    a.seg[s].x = xs[s];
    a.seg[s].dx = dxs ? dxs[s] : nullptr;
    a.seg[s].k = ks[s];
    a.seg[s].off = a.k_total;
    a.k_total += ks[s];
    *vec = *vec && ks[s] % 4 == 0 && aligned16(xs[s]);
  }
  *vec = *vec && aligned16(w);
  a.w = w;
  a.ldw = a.k_total;
  a.n = n_rows;
  a.h = h;
  return HGNN_OK;
}

struct FwdCall {
  LinArgs a;
  bool vec_in;   // fill_args' part of vec
  bool vec;      // every pointer the kernels read or write as float4 is 16-B aligned
  hipStream_t stream;
};

static void fwd_set_vec(FwdCall& c) {
  c.vec = c.vec_in && aligned16(c.a.out) && aligned16(c.a.bias) && aligned16(c.a.add);
}

// hgnn_linear_fwd_mask's arguments, checked: its error, or c for fwd_path / run_fwd (unless n = 0)
static int prepare_fwd(FwdCall& c, int32_t n_seg, const float* const* xs, const int32_t* ks,
                       int64_t n_rows, const float* w, int32_t h, const float* bias,
                       const float* add, int32_t relu, float* out, uint32_t* mask,
                       hipStream_t stream) {
  c = FwdCall{};
  c.stream = stream;
  if (int rc = fill_args(c.a, n_seg, xs, ks, nullptr, n_rows, w, h, &c.vec_in)) return rc;
  if (mask && (!relu || h % 16 != 0 || h > 128))
    return fail(HGNN_E_ARG, "linear_fwd_mask: the bit mask needs relu, h %% 16 == 0, h <= 128 (h=%d)",
                h);
  if (n_rows == 0) return HGNN_OK;
  if (!out) return fail(HGNN_E_ARG, "linear_fwd: out is null");
  c.a.bias = bias;
  c.a.add = add;
  c.a.out = out;
  c.a.relu = relu;
  c.a.mask_out = mask;
  fwd_set_vec(c);
  return HGNN_OK;
}

enum class FwdPath {
  SplitWide,     // K = 384 / 512 as two column blocks of the split kernels
  Split,         // the split kernels, H = 128, K = 128 / 256
  V4,            // the persistent f32-input kernel
  General,       // k_linear_fwd
  GeneralMask,   // no persistent kernel for the shape: the output first, then its mask from it
  ProjAdd,       // no persistent kernel to add the rows: the projection, then act(out + add)
};

static FwdPath fwd_path(const FwdCall& c) {
  const LinArgs& a = c.a;
  if (xs_wide_ok(a, c.vec) && !out_overlaps_inputs(a)) return FwdPath::SplitWide;
  const bool v4 = v4_ok(a, c.vec);
  if (a.mask_out && !v4) return FwdPath::GeneralMask;
  if (a.add && !v4) return FwdPath::ProjAdd;
  if (v4) return split_shape(a) ? FwdPath::Split : FwdPath::V4;
  return FwdPath::General;
}

static int xs_fwd_wide(const LinArgs& a, hipStream_t stream) {
  for (int part = 0; part < 2; ++part) {
    const ColBlock b = column_block(a, part);
    if (int rc = xs_linear_fwd(b.a, b.tab, stream)) return rc;
  }
  return HGNN_OK;
}

static int run_fwd(const FwdCall& c) {
  FwdCall p = c;   // the projection that is launched
  FwdPath path = fwd_path(p);
  const bool mask_after = path == FwdPath::GeneralMask;
  if (mask_after) {
    p.a.mask_out = nullptr;
    path = fwd_path(p);   // General or ProjAdd
  }
  const bool add_after = path == FwdPath::ProjAdd;
  if (add_after) {   // without the added rows and their alignment any of the kernels may take it
    p.a.add = nullptr;
    p.a.relu = 0;
    fwd_set_vec(p);
    path = fwd_path(p);
  }
  const LinArgs& a = p.a;
  int rc;
  switch (path) {
    case FwdPath::SplitWide: rc = xs_fwd_wide(a, p.stream); break;
    case FwdPath::Split: rc = xs_linear_fwd(a, chunk_table(a), p.stream); break;
    case FwdPath::V4: rc = v4_linear_fwd(a, chunk_table(a), p.stream); break;
    default: rc = gen_linear_fwd(a, p.vec, p.stream); break;
  }
  if (rc) return rc;
  if (add_after) {   // act(out + add) in one streaming pass
    const float* ins[2] = {c.a.out, c.a.add};
    const float ones[2] = {1.f, 1.f};
    if (int rc2 = hgnn_hetero_epilogue(2, ins, ones, a.n * a.h, c.a.relu, c.a.out, p.stream))
      return rc2;
  }
  if (mask_after) {
    hipLaunchKernelGGL(k_relu_mask, dim3((unsigned)cdiv(a.n * 4, 256)), dim3(256), 0, p.stream,
                       c.a.out, a.n, a.h, c.a.mask_out);
    return check_launch("k_relu_mask");
  }
  return HGNN_OK;
}

struct BwdCall {
  LinArgs a;
  bool vec_in, vec;   // as in FwdCall
  bool any_dx;        // some segment's dX is wanted
  bool wg;            // dW or db is wanted
  float *dw, *db;
  void* ws;
  size_t ws_bytes;
  hipStream_t stream;
};

static void bwd_set_vec(BwdCall& c) {
  c.vec = c.vec_in && aligned16(c.a.dout) && aligned16(c.a.out_act) && aligned16(c.a.dz_out);
  for (int s = 0; s < c.a.n_seg; ++s) c.vec = c.vec && aligned16(c.a.seg[s].dx);
}

// hgnn_linear_bwd_ex's arguments, checked: its error, or c for bwd_path / run_bwd
static int prepare_bwd(BwdCall& c, int32_t n_seg, const float* const* xs, const int32_t* ks,
                       int64_t n_rows, const float* w, int32_t h, const float* dout,
                       const float* out, const uint32_t* mask, float* const* dxs,
                       uint32_t dx_accumulate, float* dw, float* db, float* dz_out, void* ws,
                       size_t ws_bytes, hipStream_t stream) {
  c = BwdCall{};
  c.stream = stream;
  LinArgs& a = c.a;
  if (int rc = fill_args(a, n_seg, xs, ks, dxs, n_rows, w, h, &c.vec_in)) return rc;
  if (dx_accumulate >> n_seg) return fail(HGNN_E_ARG, "linear_bwd: accumulate bits beyond n_seg");
  a.dx_acc = dx_accumulate;
  if (!dout && n_rows > 0) return fail(HGNN_E_ARG, "linear_bwd: dout is null");
  if (mask && (!out || h % 16 != 0 || h > 128))
    return fail(HGNN_E_ARG, "linear_bwd_mask: the bit mask needs `out` too, h %% 16 == 0, h <= 128");
  a.dout = dout;
  a.out_act = out;
  // the persistent kernels read the bits; the others (and the streaming dz pass) read `out`
  a.mask_in = mask;
  a.dz_out = dz_out;
  bwd_set_vec(c);
  for (int s = 0; s < n_seg; ++s) c.any_dx |= a.seg[s].dx != nullptr;
  c.wg = dw || db;
  c.dw = dw;
  c.db = db;
  c.ws = ws;
  c.ws_bytes = ws_bytes;
  return HGNN_OK;
}

enum class BwdPath {
  DzPrepass,   // dz_out where no persistent dgrad writes it: a streaming pass, then planned again
  SplitWide,   // K = 384 / 512 as two column blocks of the split kernels
  Split,       // the split kernels, H = 128, K = 128 / 256
  V4,          // the persistent f32-input kernels (fused, or dgrad v4 / v5 + wgrad v4 / v5)
  Lds,         // k_linear_bwd_lds
  General,     // k_linear_dgrad + k_linear_wgrad
};

static BwdPath bwd_path(const BwdCall& c) {
  const LinArgs& a = c.a;
  const bool v4 = v4_ok(a, c.vec);
  if (a.dz_out && !(v4 && c.any_dx)) return BwdPath::DzPrepass;
  if (xs_wide_ok(a, c.vec) && (c.ws || !c.wg)) return BwdPath::SplitWide;
  if (v4) return split_shape(a) ? BwdPath::Split : BwdPath::V4;
  if (lds_bwd_ok(a, c.vec) && c.wg && c.ws) return BwdPath::Lds;
  return BwdPath::General;
}

// the split-once kernels (linear_xs.hip): dz split once for the dgrad and the wgrad; wide: the
// two column blocks of K = 384 / 512, into one slab
static int split_linear_bwd(LinArgs a, bool wide, bool dx, bool wg, void* ws, size_t ws_bytes,
                            int64_t* slabs, hipStream_t stream) {
  if (wg && (!ws || ws_bytes < split_slab_bytes(a)))
    return fail(HGNN_E_WS, "linear_bwd: workspace too small");
  a.slab = wg ? static_cast<float*>(ws) : nullptr;
  int G = 0, rc = HGNN_OK;
  for (int part = 0; part < (wide ? 2 : 1) && !rc; ++part) {
    const ColBlock b = wide ? column_block(a, part) : ColBlock{a, chunk_table(a), dx};
    if (b.dx || wg) rc = xs_linear_bwd(b.a, b.tab, b.dx, &G, stream);
  }
  *slabs = G;
  return rc;
}

static int run_bwd(BwdCall p) {
  LinArgs& a = p.a;
  if (a.n == 0) {  // no rows: weight grads are zero
    if (p.dw) (void)hipMemsetAsync(p.dw, 0, (size_t)a.h * a.k_total * 4, p.stream);
    if (p.db) (void)hipMemsetAsync(p.db, 0, (size_t)a.h * 4, p.stream);
    return check_launch("linear_bwd(n=0)");
  }
  BwdPath path = bwd_path(p);
  if (path == BwdPath::DzPrepass) {
    // dz written by a streaming pass, then the backward from it with no mask left to apply
    const float one = 1.f;
    float* dz = a.dz_out;
    if (int rc = hgnn_hetero_epilogue_bwd(1, &one, a.n * a.h, a.out_act ? 1 : 0, a.out_act,
                                          a.dout, &dz, p.stream))
      return rc;
    a.dout = dz;
    a.out_act = nullptr;
    a.mask_in = nullptr;
    a.dz_out = nullptr;
    bwd_set_vec(p);
    path = bwd_path(p);
  }
  int64_t slabs = 0;
  int rc;
  switch (path) {
    case BwdPath::SplitWide:
    case BwdPath::Split:
      rc = split_linear_bwd(a, path == BwdPath::SplitWide, p.any_dx, p.wg, p.ws, p.ws_bytes, &slabs,
                            p.stream);
      break;
    case BwdPath::V4:
      rc = v4_linear_bwd(a, chunk_table(a), p.any_dx, p.wg, p.ws, p.ws_bytes, &slabs, p.stream);
      break;
    case BwdPath::Lds:
      rc = lds_linear_bwd(a, p.any_dx, p.ws, p.ws_bytes, &slabs, p.stream);
      break;
    default:
      rc = gen_linear_bwd(a, p.vec, p.any_dx, p.wg, p.ws, p.ws_bytes, &slabs, p.stream);
      break;
  }
  if (rc || !p.wg) return rc;
  return reduce_slab(p.ws, slabs, a.h, a.k_total, p.dw, p.db, p.stream);
}

// ---- two jobs per launch (the two destination types of a sampled layer) ----
// Both jobs on the K = 384 / 512 split path with the same K: each column block is one launch for
// both (k_lin_fwd_xs2 / k_lin_bwd_xs2) and the backward's two slabs one reduce (k_wgrad_reduce2),
// 5 launches where job by job takes 10.

// byte range [p, p + bytes) against [q, q + qbytes)
static bool ranges_overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
  if (!p || !q) return false;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), q0 = reinterpret_cast<uintptr_t>(q);
  return p0 < q0 + qbytes && q0 < p0 + bytes;
}

// what job `a` reads, against a range job `b` writes (the jobs run side by side in a pair)
static bool reads_overlap(const LinArgs& a, const void* p, size_t bytes) {
  const size_t rows = (size_t)a.n * 4;
  for (int s = 0; s < a.n_seg; ++s)
    if (ranges_overlap(a.seg[s].x, rows * a.seg[s].k, p, bytes) ||
        ranges_overlap(a.seg[s].dx, rows * a.seg[s].k, p, bytes))
      return true;
  return ranges_overlap(a.add, rows * a.h, p, bytes) || ranges_overlap(a.dout, rows * a.h, p, bytes) ||
         ranges_overlap(a.out_act, rows * a.h, p, bytes) ||
         ranges_overlap(a.mask_in, rows * 4, p, bytes) ||
         ranges_overlap(a.out, rows * a.h, p, bytes);
}

static bool writes_hit(const LinArgs& w, const LinArgs& r) {
  const size_t rows = (size_t)w.n * 4;
  if (reads_overlap(r, w.out, rows * w.h) || reads_overlap(r, w.mask_out, rows * 4)) return true;
  for (int s = 0; s < w.n_seg; ++s)
    if (reads_overlap(r, w.seg[s].dx, rows * w.seg[s].k)) return true;
  return false;
}

// two jobs, each on the SplitWide path by itself, that one launch per column block can serve
static bool pairable(const LinArgs& a0, const LinArgs& a1) {
  return a0.k_total == a1.k_total && !writes_hit(a0, a1) && !writes_hit(a1, a0);
}

static int xs_fwd_wide2(const LinArgs (&a)[2], hipStream_t stream) {
  for (int part = 0; part < 2; ++part) {
    LinArgs pa[2];
    ChunkTab pt[2];
    for (int j = 0; j < 2; ++j) {
      const ColBlock b = column_block(a[j], part);
      pa[j] = b.a;
      pt[j] = b.tab;
    }
    if (int rc = xs_linear_fwd2(pa, pt, stream)) return rc;
  }
  return HGNN_OK;
}

// The backward's column blocks of both jobs (a[j].slab: job j's workspace, or null without
// weight gradients).  *launched = false, and nothing run, when the jobs' kernel variants differ.
static int xs_bwd_wide2(const LinArgs (&a)[2], float* const (&dw)[2], float* const (&db)[2],
                        bool* launched, hipStream_t stream) {
  LinArgs pa[2][2];
  ChunkTab pt[2][2];
  bool pdx[2];
  *launched = false;
  for (int part = 0; part < 2; ++part) {
    int cls[2];
    for (int j = 0; j < 2; ++j) {
      const ColBlock b = column_block(a[j], part);
      pa[part][j] = b.a;
      pt[part][j] = b.tab;
      pdx[part] = b.dx;
      cls[j] = xs_bwd_class(b.a, b.tab, b.dx);
    }
    if (cls[0] != cls[1]) return HGNN_OK;
  }
  *launched = true;
  const bool wg = a[0].slab != nullptr;
  int G[2] = {0, 0};
  for (int part = 0; part < 2; ++part) {
    if (pdx[part] || wg) {
      if (int rc = xs_linear_bwd2(pa[part], pt[part], pdx[part], G, stream)) return rc;
    }
  }
  if (!wg) return HGNN_OK;
  const int K = a[0].k_total, h = a[0].h;
  ReducePair r;
  for (int j = 0; j < 2; ++j) {
    r.slab[j] = a[j].slab;
    r.nb[j] = G[j];
    r.dw[j] = dw[j];
    r.db[j] = db[j];
  }
  r.nblk0 = cdiv((int64_t)h * (K + 1), 64);
  r.h = h;
  r.kext = K + 1;
  r.ldd = K;
  hipLaunchKernelGGL(k_wgrad_reduce2, dim3((unsigned)(2 * r.nblk0)), dim3(1024), 0, stream, r);
  return check_launch("k_wgrad_reduce2");
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_linear_fwd_multi(int32_t n_jobs, const int32_t* n_seg, const float* const* xs,
                          const int32_t* ks, const int64_t* n_rows, const float* const* w,
                          int32_t h, const float* const* bias, const int32_t* relu,
                          float* const* out, uint32_t* const* mask, hgnn_stream_t stream_) {
  if (n_jobs < 0 || (n_jobs > 0 && (!n_seg || !xs || !ks || !n_rows || !w || !out)))
    return fail(HGNN_E_ARG, "linear_fwd_multi: bad arguments");
  for (int j = 0; j < n_jobs; ++j)
    if (n_seg[j] < 1 || n_seg[j] > HGNN_MAX_SEG)
      return fail(HGNN_E_ARG, "linear_fwd_multi: job %d has n_seg=%d", j, n_seg[j]);
  hipStream_t stream = as_stream(stream_);
  if (n_jobs == 2) {   // a job the single call would refuse is refused by the loop below
    FwdCall c[2];
    bool ok = true;
    for (int j = 0, o = 0; j < 2 && ok; o += n_seg[j], ++j)
      ok = prepare_fwd(c[j], n_seg[j], xs + o, ks + o, n_rows[j], w[j], h,
                       bias ? bias[j] : nullptr, nullptr, relu ? relu[j] : 0, out[j],
                       mask ? mask[j] : nullptr, stream) == HGNN_OK &&
           c[j].a.n > 0 && fwd_path(c[j]) == FwdPath::SplitWide;
    if (ok && pairable(c[0].a, c[1].a)) {
      const LinArgs a[2] = {c[0].a, c[1].a};
      return xs_fwd_wide2(a, stream);
    }
  }
  for (int j = 0, o = 0; j < n_jobs; o += n_seg[j], ++j)
    if (int rc = hgnn_linear_fwd_mask(n_seg[j], xs + o, ks + o, n_rows[j], w[j], h,
                                      bias ? bias[j] : nullptr, nullptr, relu ? relu[j] : 0,
                                      out[j], mask ? mask[j] : nullptr, stream_))
      return rc;
  return HGNN_OK;
}

size_t hgnn_linear_bwd_multi_ws_bytes(int32_t n_jobs, const int64_t* n_rows,
                                      const int32_t* k_total, int32_t h) {
  size_t total = 0;
  for (int j = 0; j < n_jobs; ++j) total += hgnn_linear_bwd_ws_bytes(n_rows[j], k_total[j], h);
  return total;
}

int hgnn_linear_bwd_multi(int32_t n_jobs, const int32_t* n_seg, const float* const* xs,
                          const int32_t* ks, const int64_t* n_rows, const float* const* w,
                          int32_t h, const float* const* dout, const float* const* out,
                          const uint32_t* const* mask, float* const* dxs,
                          const uint32_t* dx_accumulate, float* const* dw, float* const* db,
                          void* ws, size_t ws_bytes, hgnn_stream_t stream_) {
  if (n_jobs < 0 || (n_jobs > 0 && (!n_seg || !xs || !ks || !n_rows || !w || !dout)))
    return fail(HGNN_E_ARG, "linear_bwd_multi: bad arguments");
  // job j's first segment, and its workspace (its hgnn_linear_bwd_ws_bytes, one job after the
  // other) at ws_off[j] .. ws_off[j + 1]
  std::vector<int> seg0((size_t)n_jobs);
  std::vector<size_t> ws_off((size_t)n_jobs + 1, 0);
  bool any_w = false;
  for (int j = 0, o = 0; j < n_jobs; o += n_seg[j], ++j) {
    if (n_seg[j] < 1 || n_seg[j] > HGNN_MAX_SEG)
      return fail(HGNN_E_ARG, "linear_bwd_multi: job %d has n_seg=%d", j, n_seg[j]);
    int32_t k = 0;
    for (int s = 0; s < n_seg[j]; ++s) k += ks[o + s];
    seg0[j] = o;
    ws_off[j + 1] = ws_off[j] + hgnn_linear_bwd_ws_bytes(n_rows[j], k, h);
    any_w = any_w || (dw && dw[j]) || (db && db[j]);
  }
  if (any_w && (!ws || ws_bytes < ws_off[n_jobs])) return fail(HGNN_E_WS, "linear_bwd_multi: workspace too small");
  hipStream_t stream = as_stream(stream_);
  auto prepare = [&](BwdCall& c, int j) {
    const int o = seg0[j];
    return prepare_bwd(c, n_seg[j], xs + o, ks + o, n_rows[j], w[j], h, dout[j],
                       out ? out[j] : nullptr, mask ? mask[j] : nullptr, dxs ? dxs + o : nullptr,
                       dx_accumulate ? dx_accumulate[j] : 0u, dw ? dw[j] : nullptr,
                       db ? db[j] : nullptr, nullptr,
                       ws ? static_cast<char*>(ws) + ws_off[j] : nullptr,
                       ws ? ws_off[j + 1] - ws_off[j] : 0, stream);
  };
  if (n_jobs == 2) {   // a job the single call would refuse is refused by the loop below
    BwdCall c[2];
    bool ok = true;
    for (int j = 0; j < 2 && ok; ++j)
      ok = prepare(c[j], j) == HGNN_OK && c[j].a.n > 0 && bwd_path(c[j]) == BwdPath::SplitWide &&
           (!c[j].wg || c[j].ws_bytes >= split_slab_bytes(c[j].a));
    if (ok && pairable(c[0].a, c[1].a)) {
      LinArgs a[2] = {c[0].a, c[1].a};
      for (int j = 0; j < 2; ++j) a[j].slab = c[j].wg ? static_cast<float*>(c[j].ws) : nullptr;
      float* const dwj[2] = {c[0].dw, c[1].dw};
      float* const dbj[2] = {c[0].db, c[1].db};
      bool launched;
      const int rc = xs_bwd_wide2(a, dwj, dbj, &launched, stream);
      if (launched) return rc;
    }
  }
  for (int j = 0; j < n_jobs; ++j) {
    BwdCall c;
    if (int rc = prepare(c, j)) return rc;
    if (int rc = run_bwd(c)) return rc;
  }
  return HGNN_OK;
}

int hgnn_linear_fwd(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                    const float* w, int32_t h, const float* bias, int32_t relu, float* out,
                    hgnn_stream_t stream_) {
  return hgnn_linear_fwd_mask(n_seg, xs, ks, n_rows, w, h, bias, nullptr, relu, out, nullptr,
                              stream_);
}

int hgnn_linear_fwd_add(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                        const float* w, int32_t h, const float* bias, const float* add,
                        int32_t relu, float* out, hgnn_stream_t stream_) {
  return hgnn_linear_fwd_mask(n_seg, xs, ks, n_rows, w, h, bias, add, relu, out, nullptr,
                              stream_);
}

int hgnn_linear_fwd_mask(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                         const float* w, int32_t h, const float* bias, const float* add,
                         int32_t relu, float* out, uint32_t* mask, hgnn_stream_t stream_) {
  FwdCall c;
  if (int rc = prepare_fwd(c, n_seg, xs, ks, n_rows, w, h, bias, add, relu, out, mask,
                           as_stream(stream_)))
    return rc;
  return c.a.n == 0 ? HGNN_OK : run_fwd(c);
}

// the slabs of whichever family a backward of these sizes takes: the largest block count
size_t hgnn_linear_bwd_ws_bytes(int64_t n_rows, int32_t k_total, int32_t h) {
  const int64_t n = n_rows < 1 ? 1 : n_rows;
  int64_t gx = gen_bwd_slabs(n, k_total, h);
  gx = std::max(gx, lds_bwd_slabs(n));
  gx = std::max(gx, v4_bwd_max_slabs());
  gx = std::max(gx, xs_bwd_grid(n));
  return align_up((size_t)gx * h * (k_total + 1) * 4, 256) + 256;
}

int hgnn_linear_bwd(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                    const float* w, int32_t h, const float* dout, const float* out,
                    float* const* dxs, float* dw, float* db, void* ws, size_t ws_bytes,
                    hgnn_stream_t stream_) {
  return hgnn_linear_bwd_ex(n_seg, xs, ks, n_rows, w, h, dout, out, nullptr, dxs, 0u, dw, db,
                            nullptr, ws, ws_bytes, stream_);
}

int hgnn_linear_bwd_dz(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                       const float* w, int32_t h, const float* dout, const float* out,
                       float* const* dxs, float* dw, float* db, float* dz_out, void* ws,
                       size_t ws_bytes, hgnn_stream_t stream_) {
  return hgnn_linear_bwd_ex(n_seg, xs, ks, n_rows, w, h, dout, out, nullptr, dxs, 0u, dw, db,
                            dz_out, ws, ws_bytes, stream_);
}

int hgnn_linear_bwd_mask(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                         const float* w, int32_t h, const float* dout, const float* out,
                         const uint32_t* mask, float* const* dxs, float* dw, float* db,
                         float* dz_out, void* ws, size_t ws_bytes, hgnn_stream_t stream_) {
  return hgnn_linear_bwd_ex(n_seg, xs, ks, n_rows, w, h, dout, out, mask, dxs, 0u, dw, db, dz_out,
                            ws, ws_bytes, stream_);
}

int hgnn_linear_bwd_ex(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                       const float* w, int32_t h, const float* dout, const float* out,
                       const uint32_t* mask, float* const* dxs, uint32_t dx_accumulate,
                       float* dw, float* db, float* dz_out, void* ws, size_t ws_bytes,
                       hgnn_stream_t stream_) {
  BwdCall c;
  if (int rc = prepare_bwd(c, n_seg, xs, ks, n_rows, w, h, dout, out, mask, dxs, dx_accumulate,
                           dw, db, dz_out, ws, ws_bytes, as_stream(stream_)))
    return rc;
  return run_bwd(c);
}

int hgnn_set_k3_split(int32_t on) {
  const int prev = x6_enabled() ? 1 : 0;
  if (on >= 0) g_k3_x6 = on ? 1 : 0;
  return prev;
}

// ---- single-input forms (the PyG Linear calls one at a time; SURVEY §8b names) ----------------
// lin(x) = x @ w^T (+ bias): PyG Linear inside SAGEConv (lin_l with bias, lin_r without).
int hgnn_linear_fwd_f32(const float* x, int64_t n_rows, int32_t k, const float* w, int32_t h,
                        const float* bias, float* out, hgnn_stream_t stream) {
  return hgnn_linear_fwd(1, &x, &k, n_rows, w, h, bias, 0, out, stream);
}

// dx = dy @ w (autograd of lin).  The dx-only backward never reads x, so dx stands in for it.
int hgnn_linear_dgrad_f32(const float* dy, int64_t n_rows, int32_t h, const float* w, int32_t k,
                          float* dx, hgnn_stream_t stream) {
  if (n_rows > 0 && !dx) return fail(HGNN_E_ARG, "linear_dgrad: dx is null");
  const float* x = dx;
  return hgnn_linear_bwd(1, &x, &k, n_rows, w, h, dy, nullptr, &dx, nullptr, nullptr, nullptr, 0,
                         stream);
}

// dw = dy^T @ x, db = colsum(dy) (db may be NULL).  ws: hgnn_linear_bwd_ws_bytes(n_rows, k, h).
// The weight-only backward never reads w (every W load sits behind the dx template flag), so dw
// stands in for it.
int hgnn_linear_wgrad_f32(const float* x, const float* dy, int64_t n_rows, int32_t k, int32_t h,
                          float* dw, float* db, void* ws, size_t ws_bytes, hgnn_stream_t stream) {
  if (!dw) return fail(HGNN_E_ARG, "linear_wgrad: dw is null");
  return hgnn_linear_bwd(1, &x, &k, n_rows, dw, h, dy, nullptr, nullptr, dw, db, ws, ws_bytes,
                         stream);
}

}  // extern "C"
