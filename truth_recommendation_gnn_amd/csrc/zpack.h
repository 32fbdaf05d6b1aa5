// Zero-packed fp32 rows: the format, and the per-lane arithmetic of the kernels that write it
// (zpack.hip) and read it (the ZP gather, gather.hip).  Plain C++ that compiles for the host as
// well, where tests/host/zpack_check.cpp runs it over every nibble at every lane position.
//
// A row of d floats (d = 64 or 128) whose entries are mostly zero bit patterns (a ReLU output)
// is stored in a slot of S = 128 * ceil((16 + 4 d + 12) / 128) bytes (d = 128: 640, d = 64: 384),
// row r at byte r * S, so every slot starts on a 128-B line:
//   bytes [0, 16)            the mask: bit c (bit c % 32 of little-endian word c / 32) is set
//                            iff the BIT PATTERN of x[r][c] is non-zero, so -0.0, denormals and
//                            NaN are stored values and the format is lossless; bits >= d are 0
//   bytes [16, 16 + 4 nnz)   the stored values, in column order
//   the rest                 never written; a reader may load it but no result may depend on it
// A row with the mean 52 non-zeros of cfg4's layer-2 user table takes 224 B: 2 lines, not 4.
//
// The reader keeps the unpacked gather's lane layout: lane sl of the row's d / 4 lanes owns
// columns 4 sl .. 4 sl + 3.  From the mask it takes pre = the set bits below column 4 sl and
// nib = its own four bits, loads 16 B at byte 16 + 4 pre (4-B aligned, may straddle a line;
// pre <= 4 sl <= d - 4, so it ends at or before byte 16 + 4 d of the slot, whatever the mask
// holds), and spreads the loaded words over its columns with selects (expand).  lane_read does
// this from the whole mask (the pack kernel, which has it in registers); lane_read_word from
// the lane's own mask word and the count of the words before it (the gather, which loads one
// word per lane and gets that count from its neighbours).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HGNN_ZP_HD __host__ __device__
#else
#define HGNN_ZP_HD
#endif

namespace hgnn {
namespace zpack {

constexpr int kMaskBytes = 16;
constexpr int kLine = 128;
constexpr int kHistBins = 6;   // lines per row: ceil((16 + 4 nnz) / 128) is 1 .. 5

HGNN_ZP_HD inline bool width_ok(int d) { return d == 64 || d == 128; }

// slot stride in bytes (0: the width has no packed form)
HGNN_ZP_HD inline int64_t slot_bytes(int d) {
  return width_ok(d) ? (int64_t)kLine * ((kMaskBytes + 4 * d + 12 + kLine - 1) / kLine) : 0;
}

HGNN_ZP_HD inline uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// 128-B lines the row's mask and values occupy
HGNN_ZP_HD inline int row_lines(int nnz) { return (kMaskBytes + 4 * nnz + kLine - 1) / kLine; }

// the four mask bits of a lane from the bit patterns of its four columns
HGNN_ZP_HD inline uint32_t nibble_of(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
  return (x0 ? 1u : 0u) | (x1 ? 2u : 0u) | (x2 ? 4u : 0u) | (x3 ? 8u : 0u);
}

// where lane sl's nibble sits in the mask: word sl / 8, shifted by 4 (sl % 8)
HGNN_ZP_HD inline int mask_word(int sl) { return sl >> 3; }
HGNN_ZP_HD inline int mask_shift(int sl) { return (sl & 7) * 4; }

struct LaneRead {
  uint32_t pre;   // stored values of the row before this lane's columns
  uint32_t nib;   // this lane's four mask bits
};

HGNN_ZP_HD inline LaneRead lane_read(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, int sl) {
  // Per mask word the bits that lie below the lane's columns (k0 .. k3): functions of sl alone,
  // so a kernel keeps them in registers across rows, and a row costs four and + popcount pairs
  // and three two-way selects, no branch.
  const int w = mask_word(sl), b = mask_shift(sl);
  const uint32_t low = (1u << b) - 1u, all = ~0u;
  const uint32_t k0 = w > 0 ? all : low;
  const uint32_t k1 = w > 1 ? all : (w == 1 ? low : 0u);
  const uint32_t k2 = w > 2 ? all : (w == 2 ? low : 0u);
  const uint32_t k3 = w == 3 ? low : 0u;
  const uint32_t lo = (w & 2) ? m2 : m0, hi = (w & 2) ? m3 : m1;
  const uint32_t mw = (w & 1) ? hi : lo;
  LaneRead r;
  r.pre = popc(m0 & k0) + popc(m1 & k1) + popc(m2 & k2) + popc(m3 & k3);
  r.nib = (mw >> b) & 15u;
  return r;
}

// lane_read for a lane that holds only its own mask word mw and was handed `below`, the set bits
// of the row's words before it (at most 32 per word).  Whatever the caller passes as `below`
// while it is such a sum of up to three popcounts, pre <= 96 + 28 and the 16-B read ends at or
// before byte 16 + 4 * 124 + 16 = 528 of the slot (d = 64, one word before: 16 + 4 * 60 + 16 =
// 272), so it cannot leave the slot.
HGNN_ZP_HD inline LaneRead lane_read_word(uint32_t mw, uint32_t below, int sl) {
  const int b = mask_shift(sl);
  LaneRead r;
  r.pre = below + popc(mw & ((1u << b) - 1u));
  r.nib = (mw >> b) & 15u;
  return r;
}

// byte offset in the slot of stored value number k of the row
HGNN_ZP_HD inline int value_byte(uint32_t k) { return kMaskBytes + 4 * (int)k; }

// stored-value number of the lane's column j (0 .. 3; only meaningful where bit j of nib is set)
HGNN_ZP_HD inline uint32_t value_index(uint32_t pre, uint32_t nib, int j) {
  return pre + popc(nib & ((1u << j) - 1u));
}

// The lane's four columns from the four words loaded at value_byte(pre).  Selects only: words
// past the lane's own values may be another lane's, or bytes nobody wrote.
HGNN_ZP_HD inline void expand(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t nib,
                              uint32_t (&v)[4]) {
  // a queue of the loaded words: a column whose bit is set takes the head and the queue moves
  // up by one (ten independent two-way selects)
  const bool b0 = nib & 1u, b1 = nib & 2u, b2 = nib & 4u, b3 = nib & 8u;
  v[0] = b0 ? t0 : 0u;
  const uint32_t p0 = b0 ? t1 : t0, p1 = b0 ? t2 : t1, p2 = b0 ? t3 : t2;
  v[1] = b1 ? p0 : 0u;
  const uint32_t q0 = b1 ? p1 : p0, q1 = b1 ? p2 : p1;
  v[2] = b2 ? q0 : 0u;
  const uint32_t r0 = b2 ? q1 : q0;
  v[3] = b3 ? r0 : 0u;
}

}  // namespace zpack
}  // namespace hgnn
