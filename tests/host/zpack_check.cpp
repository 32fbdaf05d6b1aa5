// Host check of the zero-packed row format (csrc/zpack.h): the pack arithmetic and the per-lane
// read arithmetic, run lane by lane as the kernels run them, on buffers of exactly n_rows * S
// bytes.  Build with -fsanitize=address,undefined and run (tests/test_zpack.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I truth_recommendation_gnn_amd/csrc \
//       tests/host/zpack_check.cpp -o zpack_check && ./zpack_check
//
// Every 16-B read must lie inside its own slot (asserted here; the sanitizer sees the last row's
// reads against the end of the allocation) and the expanded columns must equal the source row
// bit for bit.  Bytes the pack never writes hold a poison pattern, so a select that let one
// through would show as a mismatch.
#include "zpack.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hgnn;

static long g_rows = 0, g_reads = 0;

#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);         \
      std::fprintf(stderr, "\n");                \
      std::exit(1);                              \
    }                                            \
  } while (0)

// a stored value that is never zero and differs per (row, column)
static uint32_t val(int r, int c) { return 0x3f800000u + (uint32_t)(r * 131 + c + 1); }

// pack rows as k_zpack does: per lane a nibble, the mask words or-ed from the nibbles, the
// prefix from lane_read of that mask, one dword store per non-zero column
static void pack(const std::vector<uint32_t>& x, int n_rows, int d, unsigned char* out) {
  const int64_t S = zpack::slot_bytes(d);
  const int lpr = d / 4;
  for (int r = 0; r < n_rows; ++r) {
    const uint32_t* row = &x[(size_t)r * d];
    unsigned char* slot = out + r * S;
    uint32_t m[4] = {0, 0, 0, 0};
    for (int sl = 0; sl < lpr; ++sl)
      m[zpack::mask_word(sl)] |= zpack::nibble_of(row[4 * sl], row[4 * sl + 1], row[4 * sl + 2],
                                                  row[4 * sl + 3])
                                 << zpack::mask_shift(sl);
    std::memcpy(slot, m, 16);
    for (int sl = 0; sl < lpr; ++sl) {
      const zpack::LaneRead L = zpack::lane_read(m[0], m[1], m[2], m[3], sl);
      const uint32_t nib = zpack::nibble_of(row[4 * sl], row[4 * sl + 1], row[4 * sl + 2],
                                            row[4 * sl + 3]);
      CHECK(nib == L.nib, "row %d lane %d: nibble %u, lane_read gives %u", r, sl, nib, L.nib);
      for (int j = 0; j < 4; ++j)
        if (nib & (1u << j)) {
          const int off = zpack::value_byte(zpack::value_index(L.pre, nib, j));
          CHECK(off >= 16 && off + 4 <= S, "row %d lane %d: store at byte %d of a %lld-B slot", r,
                sl, off, (long long)S);
          std::memcpy(slot + off, &row[4 * sl + j], 4);
        }
    }
  }
}

// read rows as the ZP gather does and compare with the source
static void read_back(const std::vector<uint32_t>& x, int n_rows, int d, const unsigned char* buf,
                      const char* what) {
  const int64_t S = zpack::slot_bytes(d);
  const int lpr = d / 4;
  for (int r = 0; r < n_rows; ++r) {
    const unsigned char* slot = buf + r * S;
    uint32_t m[4];
    std::memcpy(m, slot, 16);
    int nnz = 0;
    for (int c = 0; c < d; ++c) nnz += x[(size_t)r * d + c] != 0;
    CHECK((int)(zpack::popc(m[0]) + zpack::popc(m[1]) + zpack::popc(m[2]) + zpack::popc(m[3])) ==
              nnz, "%s: row %d mask count", what, r);
    for (int sl = 0; sl < lpr; ++sl) {
      const zpack::LaneRead L = zpack::lane_read(m[0], m[1], m[2], m[3], sl);
      // the gather's form: the lane's own word, and the set bits of the words before it
      uint32_t below = 0;
      for (int k = 0; k < zpack::mask_word(sl); ++k) below += zpack::popc(m[k]);
      const zpack::LaneRead W = zpack::lane_read_word(m[zpack::mask_word(sl)], below, sl);
      CHECK(W.pre == L.pre && W.nib == L.nib, "%s: row %d lane %d: lane_read_word (%u, %u), "
            "lane_read (%u, %u)", what, r, sl, W.pre, W.nib, L.pre, L.nib);
      const int off = zpack::value_byte(L.pre);
      CHECK(off % 4 == 0 && off >= 16 && off + 16 <= S,
            "%s: row %d lane %d reads bytes [%d, %d) of a %lld-B slot", what, r, sl, off, off + 16,
            (long long)S);
      uint32_t t[4], v[4];
      std::memcpy(t, slot + off, 16);   // (the last row: against the end of the allocation)
      zpack::expand(t[0], t[1], t[2], t[3], L.nib, v);
      for (int j = 0; j < 4; ++j)
        CHECK(v[j] == x[(size_t)r * d + 4 * sl + j], "%s: row %d column %d: %08x, source %08x",
              what, r, 4 * sl + j, v[j], x[(size_t)r * d + 4 * sl + j]);
      ++g_reads;
    }
    ++g_rows;
  }
}

static void run(const std::vector<uint32_t>& x, int n_rows, int d, const char* what) {
  const int64_t S = zpack::slot_bytes(d);
  CHECK(S == (d == 128 ? 640 : 384), "slot_bytes(%d) = %lld", d, (long long)S);
  // exactly n_rows * S bytes on the heap: one byte past the last slot is the sanitizer's
  unsigned char* buf = static_cast<unsigned char*>(std::malloc((size_t)n_rows * S));
  CHECK(buf != nullptr, "malloc");
  std::memset(buf, 0xA5, (size_t)n_rows * S);   // poison: what the pack leaves unwritten
  pack(x, n_rows, d, buf);
  read_back(x, n_rows, d, buf, what);
  std::free(buf);
}

// a lane reading garbage as its mask (an edge slot past the segment's end reads some row's mask
// with its nibble forced to 0) still stays in the slot: pre <= 4 sl for ANY mask
static int k_of(int it, int sl) { return (it + sl) & 3; }

static void any_mask_in_slot(int d) {
  const int64_t S = zpack::slot_bytes(d);
  uint32_t s = 12345u;
  for (int it = 0; it < 20000; ++it) {
    uint32_t m[4];
    for (int k = 0; k < 4; ++k) {
      s = s * 1664525u + 1013904223u;
      m[k] = it == 0 ? 0xffffffffu : s;
    }
    for (int sl = 0; sl < d / 4; ++sl) {
      const zpack::LaneRead L = zpack::lane_read(m[0], m[1], m[2], m[3], sl);
      CHECK((int)L.pre <= 4 * sl && zpack::value_byte(L.pre) + 16 <= S, "d=%d lane %d: pre %u", d,
            sl, L.pre);
      // lane_read_word with ANY three popcounts as `below` (d = 64: one), not only the right ones
      const uint32_t worst = d == 128 ? 96u : 32u;
      for (uint32_t below : {0u, zpack::popc(m[1]) + zpack::popc(m[2]) + zpack::popc(m[3]), worst}) {
        if (below > worst) below = worst;
        const zpack::LaneRead W = zpack::lane_read_word(m[k_of(it, sl)], below, sl);
        CHECK(zpack::value_byte(W.pre) + 16 <= S, "d=%d lane %d: below %u pre %u", d, sl, below,
              W.pre);
      }
    }
  }
}

int main() {
  for (int d : {64, 128}) {
    const int lpr = d / 4;
    // every nibble at every lane position, over three backgrounds (the other lanes all zero,
    // all set, alternating), so every prefix a lane can see before a nibble occurs
    {
      std::vector<uint32_t> x;
      int r = 0;
      for (int bg = 0; bg < 3; ++bg)
        for (int sl = 0; sl < lpr; ++sl)
          for (uint32_t nib = 0; nib < 16; ++nib, ++r) {
            x.resize((size_t)(r + 1) * d);
            for (int c = 0; c < d; ++c) {
              bool on = bg == 1 || (bg == 2 && ((c * 7 + sl) % 3 == 0));
              if (c / 4 == sl) on = (nib >> (c % 4)) & 1u;
              x[(size_t)r * d + c] = on ? val(r, c) : 0u;
            }
          }
      run(x, r, d, "nibbles");
    }
    // the named masks; the LAST row of the buffer is in turn each of them
    {
      const int counts[] = {0, d, 28, 29, 60, 61, 1, d - 1};
      for (int last = 0; last < 8; ++last) {
        std::vector<uint32_t> x;
        int r = 0;
        for (int pass = 0; pass < 2; ++pass)           // non-zeros first / non-zeros last
          for (int k = 0; k < 8; ++k, ++r) {
            const int nnz = counts[(k + last + 1) % 8];
            x.resize((size_t)(r + 1) * d);
            for (int c = 0; c < d; ++c) {
              const bool on = pass == 0 ? c < nnz : c >= d - nnz;
              x[(size_t)r * d + c] = on ? val(r, c) : 0u;
            }
          }
        // spread variants of the same counts: every (d / nnz)-th column
        for (int k = 0; k < 8; ++k, ++r) {
          const int nnz = counts[(k + last + 1) % 8];
          x.resize((size_t)(r + 1) * d);
          int left = nnz;
          for (int c = 0; c < d; ++c) {
            const bool on = left > 0 && (d - c == left || (c * nnz) % d < nnz);
            if (on) --left;
            x[(size_t)r * d + c] = on ? val(r, c) : 0u;
          }
        }
        CHECK(r == 24, "rows");
        run(x, r, d, "named masks");
      }
    }
    // values whose bit pattern is non-zero though they compare equal to zero, or are not numbers
    {
      std::vector<uint32_t> x((size_t)2 * d, 0u);
      x[3] = 0x80000000u;            // -0.0
      x[4] = 0x00000001u;            // the smallest denormal
      x[d - 1] = 0x7fc00000u;        // NaN
      x[d + d - 1] = 0x80000000u;    // the last row's last column
      run(x, 2, d, "special values");
    }
    // a single row: first and last at once
    {
      std::vector<uint32_t> x((size_t)d);
      for (int c = 0; c < d; ++c) x[c] = val(0, c);
      run(x, 1, d, "one dense row");
    }
    any_mask_in_slot(d);
  }
  std::printf("zpack_check ok: %ld rows, %ld lane reads\n", g_rows, g_reads);
  return 0;
}
