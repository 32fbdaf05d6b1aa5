// Zero-packing of fp32 rows (zpack.h): one streaming pass that turns a table whose rows are
// mostly zero bit patterns (a ReLU output) into mask + stored values, for the gathers that read
// a row once per edge (the loss's dP gather, hgnn_score_gather2_zp).
//
// Mapping: one row per group of LPR = d / 4 lanes, lane sl holding columns 4 sl .. 4 sl + 3 (the
// gather's own lane layout).  The lanes' nibbles are or-ed into the row's mask words with
// shuffles, every lane takes its prefix from popcounts of that mask (zpack::lane_read, the very
// function the reader uses) and writes its non-zero words with plain dword stores.
#include "hgnn_common.h"
#include "zpack.h"

#include <stdlib.h>
#include <string.h>

namespace hgnn {

template <int LPR>
__global__ void __launch_bounds__(256) k_zpack(const float* __restrict__ x, const int64_t n_rows,
                                               unsigned char* __restrict__ out,
                                               unsigned long long* __restrict__ hist) {
  constexpr int D = LPR * 4;
  constexpr int RPB = 256 / LPR;   // rows per block
  __shared__ unsigned int h[zpack::kHistBins];
  if (hist) {
    if (threadIdx.x < zpack::kHistBins) h[threadIdx.x] = 0;
    __syncthreads();
  }
  const int sl = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const bool live = r < n_rows;
  uint4 xv = make_uint4(0u, 0u, 0u, 0u);
  if (live) xv = *reinterpret_cast<const uint4*>(x + r * D + 4 * sl);
  const uint32_t nib = zpack::nibble_of(xv.x, xv.y, xv.z, xv.w);
  // the mask word of each aligned group of 8 lanes, then the row's words from its lanes 0, 8, ..
  uint32_t w = nib << zpack::mask_shift(sl);
  w |= __shfl_xor(w, 1, 64);
  w |= __shfl_xor(w, 2, 64);
  w |= __shfl_xor(w, 4, 64);
  const int g0 = (threadIdx.x & 63) - sl;
  const uint32_t m0 = __shfl(w, g0, 64), m1 = __shfl(w, g0 + 8, 64);
  const uint32_t m2 = LPR > 16 ? __shfl(w, g0 + 16, 64) : 0u;
  const uint32_t m3 = LPR > 16 ? __shfl(w, g0 + 24, 64) : 0u;
  const zpack::LaneRead L = zpack::lane_read(m0, m1, m2, m3, sl);
  if (live) {
    unsigned char* slot = out + r * zpack::slot_bytes(D);
    if (sl == 0) *reinterpret_cast<uint4*>(slot) = make_uint4(m0, m1, m2, m3);
    const uint32_t xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (nib & (1u << j))
        *reinterpret_cast<uint32_t*>(slot + zpack::value_byte(zpack::value_index(L.pre, nib, j))) =
            xs[j];
  }
  if (hist) {
    if (live && sl == 0) {
      const int nnz = (int)(zpack::popc(m0) + zpack::popc(m1) + zpack::popc(m2) + zpack::popc(m3));
      atomicAdd(&h[zpack::row_lines(nnz)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < zpack::kHistBins && h[threadIdx.x])
      atomicAdd(hist + threadIdx.x, (unsigned long long)h[threadIdx.x]);
  }
}

// HGNN_ZPACK=auto|0|1 (default auto), read per call as HGNN_HOT_ROWS is.  auto: a fused-ReLU K3
// output (the caller knows) of at least 1 GiB, the size above which the dP gather already
// streams its rows with nt loads (gather.hip, kNtBytes): cfg4's 4.6 GB user table, not cfg2's or
// cfg3's, which the Infinity Cache holds and where the pack pass would only add a launch.
constexpr int64_t kZpackBytes = int64_t(1) << 30;
static bool zpack_policy(int64_t table_bytes, int d, bool relu_out) {
  if (!zpack::width_ok(d)) return false;
  const char* e = getenv("HGNN_ZPACK");
  if (e && !strcmp(e, "0")) return false;
  if (e && !strcmp(e, "1")) return true;
  return relu_out && table_bytes >= kZpackBytes;
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int64_t hgnn_zpack_slot_bytes(int32_t d) { return zpack::slot_bytes(d); }

int32_t hgnn_zpack_policy(int64_t table_bytes, int32_t d, int32_t relu_out) {
  return zpack_policy(table_bytes, d, relu_out != 0) ? 1 : 0;
}

int hgnn_zpack_rows(const float* x, int64_t n_rows, int32_t d, void* out, int64_t* hist,
                    hgnn_stream_t stream) {
  if (!zpack::width_ok(d)) return fail(HGNN_E_UNSUPPORTED, "zpack_rows: d=%d (64 or 128)", d);
  if (n_rows < 0) return fail(HGNN_E_ARG, "zpack_rows: n_rows=%lld", (long long)n_rows);
  if (n_rows == 0) return HGNN_OK;
  if (!x || !out) return fail(HGNN_E_ARG, "zpack_rows: null x/out");
  unsigned char* o = static_cast<unsigned char*>(out);
  unsigned long long* hg = reinterpret_cast<unsigned long long*>(hist);
  const dim3 block(256);
  if (d == 64) {
    const dim3 grid((unsigned)cdiv(n_rows, 256 / 16));
    hipLaunchKernelGGL(k_zpack<16>, grid, block, 0, as_stream(stream), x, n_rows, o, hg);
  } else {
    const dim3 grid((unsigned)cdiv(n_rows, 256 / 32));
    hipLaunchKernelGGL(k_zpack<32>, grid, block, 0, as_stream(stream), x, n_rows, o, hg);
  }
  return check_launch("k_zpack");
}

}  // extern "C"
