// Host check of csrc/softmax_online.h (the scalar state of the softmax scoring pass) against a
// two-pass float64 softmax.  Built with -fsanitize=address,undefined and run stand-alone by
// tests/test_loss_softmax.py; prints "softmax_online_check ok".
//
// Over random score sets of 2 .. 64 entries (entry 0 the positive), with spreads from +-1 to
// +-200, sets whose maximum arrives last, and sets with masked entries:
//   * the coefficients of an edge (positive plus negatives) sum to 0 to rounding;
//   * every coefficient equals the two-pass float64 one to 1e-6 of the edge's scale g / tau (the
//     size of the largest coefficient an edge can have), the loss term to 1e-6 of the
//     largest of 1, |m|, |z_0| and itself (its float operands);
//   * every row-sum factor (Step::rescale, Step::w) is in [0, 1]: nothing was exponentiated
//     unshifted.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "softmax_online.h"

using namespace hgnn::softmax;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static double uniform01() {   // splitmix64
  uint64_t x = (g_state += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (double)(x >> 11) / 9007199254740992.0;
}

static int g_fail = 0;
static double g_worst_coef = 0.0, g_worst_sum = 0.0, g_worst_loss = 0.0;

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (g_fail < 20) {                       \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                   \
        printf("\n");                          \
      }                                        \
      ++g_fail;                                \
    }                                          \
  } while (0)

// one edge: z[0] the positive, z[j] the negatives (masked where mask[j]); g and tau its scales
static void check_set(const std::vector<float>& z, const std::vector<char>& mask, float g,
                      float tau) {
  const int n = (int)z.size();
  const float inv_tau = 1.f / tau;
  // the kernel's order: open with the positive, the negatives in sequence, close, then convert
  // the parked logits
  State st = open(z[0]);
  std::vector<float> parked(n);
  parked[0] = z[0];
  for (int j = 1; j < n; ++j) {
    const float zj = mask[j] ? masked() : z[j];
    const Step s = update(st, zj);
    CHECK(s.rescale >= 0.f && s.rescale <= 1.f && s.w >= 0.f && s.w <= 1.f,
          "step factors (%g, %g) outside [0, 1]", (double)s.rescale, (double)s.w);
    if (mask[j]) CHECK(s.w == 0.f && s.rescale == 1.f, "a masked entry moved the state");
    parked[j] = zj;
  }
  const Closed c = close(st, g, inv_tau);
  CHECK(isfinite(c.loss) && isfinite(c.G) && isfinite(c.pos), "closed state not finite");
  // two-pass float64
  double m = z[0];
  for (int j = 1; j < n; ++j)
    if (!mask[j] && z[j] > m) m = z[j];
  double l = 0.0;
  for (int j = 0; j < n; ++j)
    if (j == 0 || !mask[j]) l += exp((double)z[j] - m);
  const double scale = (double)g / (double)tau;
  const double lse = m + log(l);
  const double ref_loss = lse - (double)z[0];
  double sum = c.pos, ref_neg_sum = 0.0;
  for (int j = 1; j < n; ++j) {
    const float cj = neg_coef(parked[j], st.m, c.G);
    const double ref = mask[j] ? 0.0 : scale * exp((double)z[j] - m) / l;
    ref_neg_sum += ref;
    if (mask[j]) CHECK(cj == 0.f, "a masked entry got the coefficient %g", (double)cj);
    const double e = fabs((double)cj - ref) / scale;
    if (e > g_worst_coef) g_worst_coef = e;
    CHECK(e <= 1e-6, "n=%d j=%d coefficient %g, two-pass %g (%.3g of the scale)", n, j,
          (double)cj, ref, e);
    sum += cj;
  }
  const double ep = fabs((double)c.pos + ref_neg_sum) / scale;   // pos = -(sum of the negatives')
  if (ep > g_worst_coef) g_worst_coef = ep;
  CHECK(ep <= 1e-6, "n=%d positive coefficient %g, two-pass %g (%.3g of the scale)", n,
        (double)c.pos, -ref_neg_sum, ep);
  // to rounding: n float additions of terms below the scale
  const double es = fabs(sum) / scale;
  if (es > g_worst_sum) g_worst_sum = es;
  CHECK(es <= n * 6e-8, "n=%d coefficients sum to %g (%.3g of the scale)", n, sum, es);
  const double el = fabs((double)c.loss - ref_loss) /
                    fmax(fmax(1.0, fabs(ref_loss)), fmax(fabs(m), fabs((double)z[0])));
  if (el > g_worst_loss) g_worst_loss = el;
  CHECK(el <= 1e-6, "n=%d loss %g, two-pass %g", n, (double)c.loss, ref_loss);
}

int main() {
  const float spreads[] = {1.f, 8.f, 40.f, 200.f};
  const float taus[] = {1.f, 0.2f, 0.05f};
  long sets = 0;
  for (int rep = 0; rep < 40; ++rep)
    for (int n = 2; n <= 64; ++n)
      for (float spread : spreads)
        for (int kind = 0; kind < 4; ++kind) {
          std::vector<float> z(n);
          std::vector<char> mask(n, 0);
          for (int j = 0; j < n; ++j) z[j] = (float)((2.0 * uniform01() - 1.0) * spread);
          if (kind == 1) {   // the maximum arrives last, far above the rest
            z[n - 1] = spread + (float)(uniform01() * spread);
          } else if (kind == 2) {   // ascending: the maximum moves at every entry
            for (int j = 1; j < n; ++j) z[j] = z[j - 1] + (float)(uniform01() * spread / 8);
          } else if (kind == 3) {   // masked entries, among them (when n > 2) the greatest logit
            int top = 1;
            for (int j = 1; j < n; ++j) {
              if (z[j] > z[top]) top = j;
              mask[j] = uniform01() < 0.3;
            }
            if (n > 2) mask[top] = 1;
          }
          const float g = (float)(0.25 + uniform01()) / 3000.f;
          check_set(z, mask, g, taus[(rep + n + kind) % 3]);
          ++sets;
        }
  // every negative masked: the edge is its positive alone, all coefficients exactly 0
  {
    std::vector<float> z = {3.5f, 100.f, -7.f};
    std::vector<char> mask = {0, 1, 1};
    State st = open(z[0]);
    update(st, masked());
    update(st, masked());
    const Closed c = close(st, 1.f, 1.f);
    CHECK(c.pos == 0.f && c.loss == 0.f, "all masked: pos %g loss %g", (double)c.pos,
          (double)c.loss);
    check_set(z, mask, 1.f, 1.f);
    ++sets;
  }
  CHECK(chunk(0) == 0 && chunk(64) == 0 && chunk(1) == 64 && chunk(8) == 64 && chunk(12) == 49 &&
            chunk(63) == 9,
        "chunk rule");
  for (int k = 1; k <= kMaxNeg; ++k)
    CHECK((lds_stride(k) & 1) && lds_stride(k) >= k + 1 && chunk(k) * lds_stride(k) <= kLdsWords,
          "k=%d stride / chunk", k);
  if (g_fail) {
    printf("softmax_online_check: %d failures\n", g_fail);
    return 1;
  }
  printf("softmax_online_check ok: %ld sets, worst coefficient %.3g, sum %.3g, loss %.3g\n", sets,
         g_worst_coef, g_worst_sum, g_worst_loss);
  return 0;
}
