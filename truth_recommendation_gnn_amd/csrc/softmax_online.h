// Sampled-softmax link loss: the scalar state of one edge's online softmax (softmax_loss.hip),
// plain C++ that compiles for the host as well, where tests/host/softmax_online_check.cpp runs it
// against a two-pass float64 softmax.
//
// An edge has 1 + k logits z_0 (the positive) .. z_k, seen once and in order.  The state keeps the
// running maximum m and, apart from each other, the positive's exponential and the negatives' sum
//   l_neg = sum_{j >= 1} exp(z_j - m)
// rescaled by exp(m_old - m_new) whenever the maximum moves, so nothing is ever exponentiated
// unshifted.  A masked entry (an out-of-range negative) is the logit -inf: its weight is 0 and the
// maximum stays.  With l = exp(z_0 - m) + l_neg the edge's term and gradient coefficients are
//   loss  = m + log l - z_0
//   pos   = -G * l_neg                 G = g / (tau * l)
//   neg_j =  G * exp(z_j - m)
// the positive's g (pi_0 - 1) / tau formed as -g (sum_{j >= 1} pi_j) / tau: no cancellation where
// pi_0 is near 1.  The coefficients of an edge sum to 0 up to the rounding of l_neg's additions.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HGNN_SM_HD __host__ __device__
#else
#define HGNN_SM_HD
#endif

namespace hgnn {
namespace softmax {

constexpr int kMaxNeg = 63;        // 1 + k logits per edge fit a 64-column row of the LDS arrays
constexpr int kLdsWords = 640;     // per wave and array, as the hard-negative miner's

// the per-position stride of the kernel's LDS arrays over 1 + k columns: odd (hardneg.hip's rule)
HGNN_SM_HD inline int lds_stride(int k) { return (k + 1) | 1; }

// positions of one user a wave takes at a time: C = min(64, words / stride(k + 1))
HGNN_SM_HD inline int chunk(int k) {
  if (k < 1 || k > kMaxNeg) return 0;
  const int c = kLdsWords / lds_stride(k);
  return c < 64 ? c : 64;
}

// exp / log of the state: the hardware transcendentals on the device (v_exp_f32 / v_log_f32)
HGNN_SM_HD inline float exp_of(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __expf(x);
#else
  return expf(x);
#endif
}
HGNN_SM_HD inline float log_of(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __logf(x);
#else
  return logf(x);
#endif
}

// the logit of a masked entry
HGNN_SM_HD inline float masked() { return -__builtin_inff(); }

struct State {
  float m;       // running maximum (finite: z_0 is)
  float l_neg;   // sum over the negatives seen of exp(z_j - m)
  float z0;      // the positive's logit
};

// the positive opens the edge
HGNN_SM_HD inline State open(float z0) { return State{z0, 0.f, z0}; }

struct Step {
  float rescale;   // exp(m_old - m_new): what the sums taken so far are multiplied by
  float w;         // exp(z - m_new): the weight of this entry in them
};

// negative logit z (or masked()) enters the state; the caller applies Step to its row sum
HGNN_SM_HD inline Step update(State& s, float z) {
  const float mn = z > s.m ? z : s.m;
  Step r;
  r.rescale = exp_of(s.m - mn);   // 1 where the maximum stays (exp_of(0) == 1)
  r.w = exp_of(z - mn);           // 0 for masked()
  s.l_neg = s.l_neg * r.rescale + r.w;
  s.m = mn;
  return r;
}

struct Closed {
  float loss;   // m + log l - z_0
  float G;      // g / (tau * l): neg_j = G * exp(z_j - m), and the row sum's factor
  float pos;    // -G * l_neg
};

// g: the edge's scale (c / E, or w_e / E); inv_tau: 1 / temperature
HGNN_SM_HD inline Closed close(const State& s, float g, float inv_tau) {
  const float p0 = exp_of(s.z0 - s.m);
  const float l = p0 + s.l_neg;
  Closed c;
  c.loss = (s.m - s.z0) + log_of(l);
  c.G = g * inv_tau / l;
  c.pos = -c.G * s.l_neg;
  return c;
}

// a parked logit's coefficient under the edge's final (m, G)
HGNN_SM_HD inline float neg_coef(float z, float m, float G) { return G * exp_of(z - m); }

}  // namespace softmax
}  // namespace hgnn
