// tsne_cells.hpp -- the per-element arithmetic that fitting a t-SNE map (tsne.hip) and placing new rows into it (tsne_place.hip)
// share, so that a placed row is weighed and moved as a fitted one is: sklearn's bisection of the precision, the Student-t
// kernel q and one gains / velocity / position step.  The sums that feed them stay with the kernels (block-wide, per lane).
#pragma once
#include "common.hpp"

namespace g2v {
namespace {

// sklearn's _binary_search_perplexity in float64: beta = 1, doubled / halved while a bound is infinite, <= TS_BISECT_STEPS steps,
// stop at |H - log(perplexity)| <= 1e-5, a row sum of exactly 0 becomes 1e-8.  The conditionals are exp(-beta_eval d^2) / sum_p:
// sklearn keeps the probabilities of the last beta it EVALUATED, not the one it would try next.
constexpr int TS_BISECT_STEPS = 100;

struct TsBisect {
  double beta = 1.0, beta_eval = 1.0, beta_min = -__builtin_inf(), beta_max = __builtin_inf(), sum_p = 1.0;
};

// s0 = sum exp(-beta d^2), s1 = sum d^2 exp(-beta d^2) at b.beta -> true: stop; false: b.beta is the next precision to evaluate
__device__ __forceinline__ bool ts_bisect_next(TsBisect& b, double s0, double s1, double log_perp) {
  b.beta_eval = b.beta;
  b.sum_p = s0 == 0.0 ? 1e-8 : s0;
  const double diff = log(b.sum_p) + b.beta * (s1 / b.sum_p) - log_perp;
  if (fabs(diff) <= 1e-5) return true;
  if (diff > 0.0) {
    b.beta_min = b.beta;
    b.beta = b.beta_max == __builtin_inf() ? b.beta * 2.0 : (b.beta + b.beta_max) * 0.5;
  } else {
    b.beta_max = b.beta;
    b.beta = b.beta_min == -__builtin_inf() ? b.beta * 0.5 : (b.beta + b.beta_min) * 0.5;
  }
  return false;
}

// q = 1 / (1 + |dy|^2) in fp32 (within 2 ulp)
__device__ __forceinline__ float ts_q(float dx, float dy) { return 1.0f / (1.0f + fmaf(dx, dx, dy * dy)); }

// one component of sklearn's _gradient_descent step in its fp32 operation order (no contraction): gains += 0.2 where
// velocity * grad < 0, *= 0.8 elsewhere, floor 0.01; velocity = momentum velocity - lr (gains grad); y += velocity.
// -> gains grad, whose norm sklearn's stop rule reads
__device__ __forceinline__ float ts_step(float g, float momentum, float lr, float& y, float& v, float& gn) {
  gn = fmaxf((__fmul_rn(v, g) < 0.f) ? __fadd_rn(gn, 0.2f) : __fmul_rn(gn, 0.8f), 0.01f);
  const float gg = __fmul_rn(g, gn);
  v = __fsub_rn(__fmul_rn(momentum, v), __fmul_rn(lr, gg));
  y = __fadd_rn(y, v);
  return gg;
}

}  // namespace
}  // namespace g2v
