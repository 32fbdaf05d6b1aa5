// The BCE link loss's per-pair terms from one exponential (scoring.hip, gather.hip; included by
// hgnn_common.h).  Plain C++ that compiles for the host as well, with libm in place of the
// hardware transcendentals, where tests/host/bce_terms_check.cpp runs it against long double.
//
// With t = exp(-|z|) in [0, 1] (0 once exp underflows) a pair's terms are
//   sigmoid(z)     = z >= 0 ? 1/(1+t) : t/(1+t)          the negatives' coefficient
//   sigmoid(z) - 1 = -sigmoid(-z)                        the positives' coefficient
//   softplus(x)    = max(x, 0) + log1p(t)                the loss term (x = -z for a positive)
// Every path of the loss forms them here, so that a saturated score keeps its relative accuracy:
// 1/(1+t) - 1 cancels (from z ~ 8 it has lost digits, from z ~ 17 it is exactly 0 and a positive
// edge pushes nothing), and log(1 + t) carries the rounding of 1 + t, 2^-24 absolute on a term of
// size t.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define HGNN_BCE_HD __host__ __device__ __forceinline__
#else
#define HGNN_BCE_HD inline
#endif

namespace hgnn {

// Hardware transcendentals on the device (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1-2 ulp).
HGNN_BCE_HD float exp_neg_abs(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __expf(-fabsf(x));
#else
  return expf(-fabsf(x));
#endif
}
HGNN_BCE_HD float bce_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.f / x;
#endif
}
HGNN_BCE_HD float bce_log(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __logf(x);
#else
  return logf(x);
#endif
}

// sigmoid(x) from t = exp_neg_abs(x)
HGNN_BCE_HD float sigmoid_t(float x, float t) {
  const float r = bce_rcp(1.f + t);
  return x >= 0.f ? r : t * r;
}

// The positives' coefficient sigmoid(z) - 1, formed as -sigmoid(-z) from the same t: a product,
// no subtraction, so it keeps its digits down to the underflow of t.
HGNN_BCE_HD float pos_coef_t(float z, float t) { return -sigmoid_t(-z, t); }

// Either coefficient where the pair's side is a run-time value (the dP gathers' weight mode):
// pos_coef_t(z, t) or sigmoid_t(z, t), bit for bit, as one sigmoid of the signed score.
HGNN_BCE_HD float pair_coef_t(bool positive, float z, float t) {
  const float s = sigmoid_t(positive ? -z : z, t);
  return positive ? -s : s;
}

// log(1 + t) for t in [0, 1] to a few ulp of the result.  u = 1 + t holds the part d = u - 1 of t
// (exact: u is in [1, 2]) and drops e = t - d (exact too: the rounding error of an addition),
// |e| <= 2^-24.  log(1 + t) = log(u) + log(1 + e / u) = log(u) + e / u up to (e / u)^2 / 2.  The
// division is left out: e - e / u = e t / (1 + t), at most 2^-24 of the result (log(1 + t) is at
// least t / (1 + t)), half an ulp, for two subtractions and an addition and nothing kept live
// that the sigmoid does not keep.  Below 2^-24, where u is 1, this is 0 + t.  It leans on log(u)
// being accurate relative to its result for u next to 1.
HGNN_BCE_HD float log1p_t(float t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float u = 1.f + t;
  const float d = u - 1.f;
  return bce_log(u) + (t - d);
}

// softplus(x) = log(1 + exp(x)) from t = exp_neg_abs(x).  The sum is a rounded add of a rounded
// product wherever this is inlined (no contraction into an fma), so that two kernels that form a
// pair's term form the same bits.
HGNN_BCE_HD float softplus_t(float x, float t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float l = log1p_t(t);
  return fmaxf(x, 0.f) + l;
}

}  // namespace hgnn
