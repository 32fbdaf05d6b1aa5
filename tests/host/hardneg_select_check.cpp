// Host check of the hard-negative selection rounds (csrc/hardneg_select.h) against a naive
// restatement of the contract in include/hgnn.h, for every M in 1 .. 64 with k in {1, 2, M}, on
// inputs that include all-equal scores, all-duplicate ids, all-positive ids, out-of-range ids,
// NaN and infinities.  Built with the address and undefined-behaviour sanitizers and run as a
// program of its own (tests/test_hard_negatives.py); every array is sized exactly, so a read or
// write past M or k is an error.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hardneg_select.h"

namespace {

uint64_t rng_state = 0x1234567ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

// The contract, pick by pick: every pick scans all columns and compares each id against every
// earlier pick (O(M * k) per pick).
int naive(const std::vector<float>& sc, const std::vector<int32_t>& ids, int k, int32_t positive,
          int64_t n_posts, std::vector<int32_t>& out) {
  const int m = (int)ids.size();
  std::vector<char> taken(m, 0);
  std::vector<int32_t> picked;   // posts of the eligible picks so far
  int n_short = 0;
  for (int r = 0; r < k; ++r) {
    int best = -1;
    double bs = 0.0;
    for (int j = 0; j < m; ++j) {
      if (taken[j]) continue;
      if (ids[j] < 0 || ids[j] >= n_posts || ids[j] == positive) continue;
      bool dup = false;
      for (int32_t p : picked) dup = dup || p == ids[j];
      if (dup) continue;
      const double s = std::isnan(sc[j]) ? -std::numeric_limits<double>::infinity()
                                         : (double)sc[j];
      if (best < 0 || s > bs) {
        best = j;
        bs = s;
      }
    }
    if (best >= 0) {
      taken[best] = 1;
      picked.push_back(ids[best]);
      out[r] = ids[best];
      continue;
    }
    ++n_short;
    int low = -1;
    for (int j = 0; j < m && low < 0; ++j)
      if (!taken[j] && ids[j] >= 0 && ids[j] < n_posts) low = j;
    if (low >= 0) {
      taken[low] = 1;
      out[r] = ids[low];
    } else {
      out[r] = positive;
    }
  }
  return n_short;
}

long n_cases = 0, n_short_cases = 0;

void check(const std::vector<float>& sc, const std::vector<int32_t>& ids, int k,
           int32_t positive, int64_t n_posts, const char* what) {
  const int m = (int)ids.size();
  std::vector<int32_t> want(k, -7), got(k, -7);
  const int ws = naive(sc, ids, k, positive, n_posts, want);
  const int gs = hgnn::hardneg::select_k(sc.data(), ids.data(), m, k, positive, n_posts,
                                         got.data());
  ++n_cases;
  n_short_cases += ws > 0;
  bool ok = ws == gs;
  for (int r = 0; r < k; ++r) {
    ok = ok && want[r] == got[r];
    ok = ok && got[r] >= 0 && got[r] < n_posts;   // every written id is a valid post
  }
  if (!ok) {
    std::printf("MISMATCH %s: M=%d k=%d positive=%d short %d vs %d\n", what, m, k, positive, gs,
                ws);
    for (int r = 0; r < k; ++r) std::printf("  pick %d: got %d want %d\n", r, got[r], want[r]);
    std::exit(1);
  }
}

}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float inf = std::numeric_limits<float>::infinity();
  for (int m = 1; m <= 64; ++m) {
    if (hgnn::hardneg::lds_stride(m) % 2 != 1 || hgnn::hardneg::lds_stride(m) < m) {
      std::printf("lds_stride(%d) = %d\n", m, hgnn::hardneg::lds_stride(m));
      return 1;
    }
    const int ks[3] = {1, 2 <= m ? 2 : 1, m};
    for (int k : ks) {
      const int64_t n_posts = 37;
      const int32_t positive = 5;
      std::vector<float> sc(m);
      std::vector<int32_t> ids(m);
      // all-equal scores over distinct ids (wrapping into duplicates past 37 columns)
      for (int j = 0; j < m; ++j) { sc[j] = 1.5f; ids[j] = (j * 7 + 3) % 37; }
      check(sc, ids, k, positive, n_posts, "equal scores");
      // all-duplicate ids
      for (int j = 0; j < m; ++j) { sc[j] = (float)(rnd() % 9) - 4.f; ids[j] = 11; }
      check(sc, ids, k, positive, n_posts, "duplicate ids");
      // every candidate is the positive
      for (int j = 0; j < m; ++j) ids[j] = positive;
      check(sc, ids, k, positive, n_posts, "all positive");
      // every candidate out of range (both sides), then a mix
      for (int j = 0; j < m; ++j) ids[j] = (j & 1) ? -1 - j : 37 + j;
      check(sc, ids, k, positive, n_posts, "all out of range");
      for (int j = 0; j < m; ++j) ids[j] = (j % 3 == 0) ? 37 : (int32_t)(rnd() % 37);
      check(sc, ids, k, positive, n_posts, "some out of range");
      // NaN everywhere, then NaN and infinities among coarse scores
      for (int j = 0; j < m; ++j) { sc[j] = nan; ids[j] = (int32_t)(rnd() % 37); }
      check(sc, ids, k, positive, n_posts, "all NaN");
      for (int j = 0; j < m; ++j) sc[j] = -inf;
      check(sc, ids, k, positive, n_posts, "all -inf");
      for (int t = 0; t < 40; ++t) {
        for (int j = 0; j < m; ++j) {
          const uint32_t c = rnd() % 16;
          sc[j] = c == 0 ? nan : c == 1 ? inf : c == 2 ? -inf : (float)(rnd() % 7) * 0.25f - 0.75f;
          // few posts and a coarse grid: ties, duplicates and own-positive candidates abound
          ids[j] = (int32_t)(rnd() % (t < 20 ? 6 : 40)) - (t % 5 == 0 ? 1 : 0);
        }
        check(sc, ids, k, (int32_t)(rnd() % 6), n_posts, "random");
      }
    }
  }
  if (n_short_cases < 100) {
    std::printf("only %ld of %ld cases fell short\n", n_short_cases, n_cases);
    return 1;
  }
  std::printf("hardneg_select_check ok: %ld cases, %ld with shortfalls\n", n_cases, n_short_cases);
  return 0;
}
