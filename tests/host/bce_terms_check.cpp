// Host check of csrc/bce_terms.h (the BCE link loss's coefficient and softplus helpers) against
// long double.  Built with -fsanitize=address,undefined and run stand-alone by
// tests/test_loss_saturation.py; prints "bce_terms_check ok".
//
// This checks the ALGEBRA of the helpers -- that -sigmoid(-z) and the corrected log1p lose no
// digits at any score -- with libm's expf / logf and an IEEE division in place of the hardware
// transcendentals.  What v_exp_f32, v_log_f32 and v_rcp_f32 add on the device (1-2 ulp each, and
// the rounding of z * log2(e)) is measured by the GPU tests of that file, not here.
//
// z sweeps [-200, 200] in steps of 1/64, plus every float within 64 ulp of +-16.6 (where
// 1 / (1 + t) - 1 reaches exactly 0), of +-87.3 (t leaves the normal range) and of +-88.7 and
// +-103.9 (t leaves the subnormal range).  Each of
//   pos_coef_t(z, t)    against  -1 / (1 + exp(z))
//   sigmoid_t(z, t)     against   1 / (1 + exp(-z))
//   softplus_t(z, t)    against   log1p(exp(z))
// must be within 8 * 2^-24 of the reference's own size (exp, 1 + t, the division, the log and
// three products at half an ulp each), plus 2^-148 where the result is subnormal, must be finite,
// and must have the reference's sign.  The forms the helpers replace are evaluated beside them and
// must FAIL that bound from z = 8 up: a check that they could pass would not tell the two apart.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bce_terms.h"

using namespace hgnn;

static int g_fail = 0;
static double g_worst_coef = 0.0, g_worst_sig = 0.0, g_worst_sp = 0.0;
static long g_old_coef_bad = 0, g_old_sp_bad = 0, g_old_seen = 0;

#define CHECK(cond, ...)                            \
  do {                                              \
    if (!(cond)) {                                  \
      if (g_fail < 20) {                            \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                        \
        printf("\n");                               \
      }                                             \
      ++g_fail;                                     \
    }                                               \
  } while (0)

static const double kRel = 8.0 / 16777216.0;   // 8 * 2^-24
static const double kSub = 0x1p-148;

// error of `got` in units of the bound at `ref`
static double ratio(float got, long double ref) {
  const double e = fabs((double)((long double)got - ref));
  return e / (kRel * fabs((double)ref) + kSub);
}

static void check_z(float z) {
  const float t = exp_neg_abs(z);
  CHECK(t >= 0.f && t <= 1.f, "z=%g: t=%g outside [0, 1]", (double)z, (double)t);
  const long double zl = z;
  const long double ref_coef = -1.0L / (1.0L + expl(zl));
  const long double ref_sig = 1.0L / (1.0L + expl(-zl));
  const long double ref_sp = zl > 0 ? zl + log1pl(expl(-zl)) : log1pl(expl(zl));
  const float coef = pos_coef_t(z, t), sig = sigmoid_t(z, t), sp = softplus_t(z, t);
  CHECK(isfinite(coef) && isfinite(sig) && isfinite(sp), "z=%g: not finite", (double)z);
  CHECK(coef <= 0.f && coef >= -1.f, "z=%g: coefficient %g outside [-1, 0]", (double)z,
        (double)coef);
  CHECK(sig >= 0.f && sig <= 1.f, "z=%g: sigmoid %g outside [0, 1]", (double)z, (double)sig);
  CHECK(sp >= 0.f, "z=%g: softplus %g negative", (double)z, (double)sp);
  const double rc = ratio(coef, ref_coef), rs = ratio(sig, ref_sig), rp = ratio(sp, ref_sp);
  if (rc > g_worst_coef) g_worst_coef = rc;
  if (rs > g_worst_sig) g_worst_sig = rs;
  if (rp > g_worst_sp) g_worst_sp = rp;
  CHECK(rc <= 1.0, "z=%g: coefficient %.9g, long double %.9Lg (%.3g of the bound)", (double)z,
        (double)coef, ref_coef, rc);
  CHECK(rs <= 1.0, "z=%g: sigmoid %.9g, long double %.9Lg (%.3g of the bound)", (double)z,
        (double)sig, ref_sig, rs);
  CHECK(rp <= 1.0, "z=%g: softplus %.9g, long double %.9Lg (%.3g of the bound)", (double)z,
        (double)sp, ref_sp, rp);
  // the two are one function of |z|: pos_coef_t(z) = -sigmoid_t(-z), bit for bit
  CHECK(coef == -sigmoid_t(-z, t), "z=%g: pos_coef_t is not -sigmoid_t(-z)", (double)z);
  // the replaced forms, where they cancel (the positive's coefficient at z >= 8; the softplus of
  // the saturated side, whose term is log1p(t) alone)
  if (z >= 8.f && z <= 80.f) {
    ++g_old_seen;
    const float old_coef = 1.f / (1.f + t) - 1.f;
    const float old_sp = fmaxf(-z, 0.f) + logf(1.f + t);
    const long double ref_sp_neg = log1pl(expl(-zl));
    if (ratio(old_coef, ref_coef) > 1.0) ++g_old_coef_bad;
    if (ratio(old_sp, ref_sp_neg) > 1.0) ++g_old_sp_bad;
    const float new_sp = softplus_t(-z, t);
    const double rn = ratio(new_sp, ref_sp_neg);
    if (rn > g_worst_sp) g_worst_sp = rn;
    CHECK(rn <= 1.0, "z=%g: softplus(-z) %.9g, long double %.9Lg", (double)z, (double)new_sp,
          ref_sp_neg);
  }
}

static void around(float z0) {
  for (int s = -1; s <= 1; s += 2) {
    float z = s * z0;
    uint32_t b;
    memcpy(&b, &z, 4);
    for (int k = -64; k <= 64; ++k) {
      const uint32_t bk = b + (uint32_t)k;
      float zk;
      memcpy(&zk, &bk, 4);
      check_z(zk);
    }
  }
}

int main() {
  long n = 0;
  for (int i = -200 * 64; i <= 200 * 64; ++i, ++n) check_z((float)i / 64.f);
  const float edges[] = {16.6f, 16.635532f /* 24 ln 2 */, 87.3f, 87.33654f /* 126 ln 2 */, 88.7f,
                         103.9f, 103.2789f /* 149 ln 2 */};
  for (float e : edges) around(e);
  // the ends: signed zeros, the largest finite score, scores far past the underflow of t
  const float ends[] = {0.f, -0.f, 1e4f, -1e4f, 3.0e38f, -3.0e38f, 1e-30f, -1e-30f};
  for (float z : ends) check_z(z);
  CHECK(pos_coef_t(0.f, 1.f) == -0.5f && sigmoid_t(-0.f, 1.f) == 0.5f, "z = 0");
  CHECK(softplus_t(1e4f, exp_neg_abs(1e4f)) == 1e4f && softplus_t(-1e4f, exp_neg_abs(1e4f)) == 0.f,
        "z = 1e4: softplus");
  CHECK(pos_coef_t(-1e4f, exp_neg_abs(1e4f)) == -1.f && pos_coef_t(1e4f, exp_neg_abs(1e4f)) == 0.f,
        "z = 1e4: coefficient");
  CHECK(log1p_t(0.f) == 0.f && log1p_t(0x1p-30f) == 0x1p-30f, "log1p_t of a t below 2^-24");
  // the replaced forms do fail where the issue says they do
  CHECK(g_old_coef_bad * 10 >= g_old_seen * 9, "1/(1+t) - 1 passed at %ld of %ld points of [8, 80]",
        g_old_seen - g_old_coef_bad, g_old_seen);
  CHECK(g_old_sp_bad * 10 >= g_old_seen * 9, "log(1 + t) passed at %ld of %ld points of [8, 80]",
        g_old_seen - g_old_sp_bad, g_old_seen);
  if (g_fail) {
    printf("bce_terms_check: %d failures\n", g_fail);
    return 1;
  }
  printf("bce_terms_check ok: %ld scores, worst of the bound: coefficient %.3g, sigmoid %.3g, "
         "softplus %.3g; the replaced forms miss it at %ld and %ld of %ld scores in [8, 80]\n",
         n, g_worst_coef, g_worst_sig, g_worst_sp, g_old_coef_bad, g_old_sp_bad, g_old_seen);
  return 0;
}
