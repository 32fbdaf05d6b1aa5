// The per-lane reads of a zero-packed row on the device (zpack.h has the format and the host-
// checkable arithmetic): the 16-B value load, the DPP move of an integer and the way a lane gets a
// row's mask.  Shared by the kernels that gather zero-packed rows (gather.hip, coef_gather.hip).
#pragma once
#include "hgnn_common.h"
#include "zpack.h"

namespace hgnn {

// 16 B at a 4-byte-aligned address (a zero-packed row's values): one dwordx4 load.  NT is a
// template flag here, not GatherArgs::nt_load read in the loop: with both forms of one load in
// an if / else the compiler merged them into a single plain load (no nt in the ISA).
typedef uint32_t zp_u4 __attribute__((ext_vector_type(4)));
typedef zp_u4 zp_u4_a4 __attribute__((aligned(4)));
template <bool NT>
__device__ __forceinline__ uint4 zp_load16(const char* p) {
  zp_u4 v;
  if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const zp_u4_a4*>(p));
  else v = *reinterpret_cast<const zp_u4_a4*>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// a DPP move of an integer; lanes without a source lane, and the rows outside ROWS, get 0
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
  // (all rows: bound_ctrl zeroes the lanes without a source and no register has to be cleared
  // first; a row mask keeps `old`, which then has to be the zero)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xF, ROWS == 0xF);
}

// How a lane of the ZP gather gets a row's mask: it loads only the mask word its own columns are
// in (one register per row in flight, a dword request), and the set bits of the row's words
// before that one come from the other lanes of the slot, which hold those words: the popcount
// moved up by 8 lanes inside a 16-lane DPP row (row_shr:8) and, in a 32-lane slot, the first
// row's total broadcast into the second (row_bcast:15 into rows 1 and 3).  Measured against every
// lane loading the whole 16-B mask (zpack::lane_read; a dwordx4 request per row, four registers)
// at cfg4: 27.3 ms against 31.4 - 35.9 ms for the gather, DESIGN.md section 5.
template <int LPR>
struct ZpMask {
  static __device__ __forceinline__ uint32_t load(const char* slot, int sl) {
    // default policy, never nt: the row's first line is wanted again at once, by the value loads
    return *reinterpret_cast<const uint32_t*>(slot + 4 * zpack::mask_word(sl));
  }
  static __device__ __forceinline__ zpack::LaneRead read(uint32_t mw, int sl) {
    const uint32_t c = zpack::popc(mw);
    const uint32_t up = dpp_u32<0x118, 0xF>(c);              // row_shr:8
    uint32_t below = up;
    if constexpr (LPR == 32) below += dpp_u32<0x142, 0xA>(c + up);   // row_bcast:15, rows 1, 3
    return zpack::lane_read_word(mw, below, sl);
  }
};

}  // namespace hgnn
