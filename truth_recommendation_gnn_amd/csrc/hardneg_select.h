// Hard-negative mining: the selection rounds of one position (hardneg.hip), plain C++ that
// compiles for the host as well, where tests/host/hardneg_select_check.cpp runs it against a
// naive restatement for every M in 1 .. 64.
//
// A position has M candidate columns (score s_j, post id c_j) and its own positive post.  Column
// j is eligible if 0 <= c_j < n_posts, c_j is not the positive, and c_j is not a post already
// picked for this position.  Pick r = 0 .. k-1 is the eligible, not yet taken column of the
// greatest score, the lowest column on equal scores; a NaN score counts as -inf.  When no
// eligible column is left the pick is a shortfall: the lowest untaken in-range column whatever
// it holds, else the positive itself.  So every id written is a valid post id, the picks of
// eligible columns are distinct posts in descending score order, and the number of shortfalls
// is returned.
//
// Two 64-bit masks carry the state (hence M <= 64): `taken` (columns picked) and `dead` (columns
// that can no longer be eligible: out of range, the positive, or a post picked before).  A round
// is one pass over the M columns that also retires the duplicates of the previous pick, so k
// picks cost k * M score/id reads, not k * k * M.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HGNN_HN_HD __host__ __device__
#else
#define HGNN_HN_HD
#endif

namespace hgnn {
namespace hardneg {

constexpr int kMaxCand = 64;

// the per-position stride of the kernel's LDS arrays: odd, so that lanes p and p + 1 .. p + 31
// fall on different banks whatever M is (a power-of-two M would put them 32 / M apart)
HGNN_HN_HD inline int lds_stride(int m) { return m | 1; }

HGNN_HN_HD inline bool in_range(int32_t id, int64_t n_posts) {
  return id >= 0 && (int64_t)id < n_posts;
}

// sc[j], ids[j] for j in [0, m): the position's candidates; out[r] for r in [0, k): its picks.
// Returns the number of shortfalls.  Requires 1 <= k <= m <= 64.
HGNN_HN_HD inline int select_k(const float* sc, const int32_t* ids, int m, int k,
                               int32_t positive, int64_t n_posts, int32_t* out) {
  uint64_t taken = 0, dead = 0, inr = 0;
  int32_t last = -1;        // the previous round's pick, to retire its duplicates (-1: none;
  bool have_last = false;   //  ids are compared only where have_last, so -1 is just a filler)
  int n_short = 0;
  for (int r = 0; r < k; ++r) {
    int best = -1;
    float bs = 0.f;
    for (int j = 0; j < m; ++j) {
      const uint64_t bit = uint64_t(1) << j;
      const int32_t id = ids[j];
      if (r == 0) {
        if (in_range(id, n_posts)) inr |= bit;
        else dead |= bit;
        if (id == positive) dead |= bit;
      } else if (have_last && id == last) {
        dead |= bit;
      }
      if ((taken | dead) & bit) continue;
      float s = sc[j];
      if (s != s) s = -__builtin_inff();
      if (best < 0 || s > bs) {
        best = j;
        bs = s;
      }
    }
    have_last = false;
    if (best >= 0) {
      taken |= uint64_t(1) << best;
      last = ids[best];
      have_last = true;
      out[r] = last;
      continue;
    }
    ++n_short;
    const uint64_t left = inr & ~taken;
    if (left) {
      const int j = __builtin_ctzll(left);
      taken |= uint64_t(1) << j;
      out[r] = ids[j];
    } else {
      out[r] = positive;
    }
  }
  return n_short;
}

}  // namespace hardneg
}  // namespace hgnn
