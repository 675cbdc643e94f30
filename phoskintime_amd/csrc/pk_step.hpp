// pk_step.hpp -- the two pieces of the adaptive step-size rule that every per-protein and network integrator shares as code: the first
// step and the clamped step-size divisor.  Plain C++ over <math.h>: device code under hipcc, host code under g++
// (tests/test_step_control_cpu.py, tests/test_step_growth_cpu.py).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PK_STEP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PK_STEP_FN inline
#endif

namespace pk {

// First step: Hairer's hinit-lite on the two max-norms d0 = |y / sc|, d1 = |f(y) / sc|; a positive h0 overrides it.
PK_STEP_FN double step_h0(double d0, double d1, double h0) {
  double h = (d0 > 1e-5 && d1 > 1e-5) ? 0.01 * d0 / d1 : 1e-6;
  if (h0 > 0.0) h = h0;
  if (!(h > 0.0) || h != h) h = 1e-6;
  return h;
}

// Step-size divisor from root = err^(1/Q): hnew = hs / fac shrinks at most 5x and grows at most 1/lo.
PK_STEP_FN double step_fac(double root, double lo = 1.0 / 6.0, double safety_inv = 1.0 / 0.9) {
  return fmax(lo, fmin(5.0, root * safety_inv));
}

// The same rule as a multiplier, from root_inv = err^(-1/Q): hnew = hs * step_growth(root_inv) grows at most hi-fold and shrinks at most
// 5x -- step_fac's clamps [1/6, 5] and its safety factor, each inverted, so that the caller needs no reciprocal (dist_fast_kernel forms
// root_inv by negating the exponent).  A NaN takes the shrinking clamp, as in step_fac.
PK_STEP_FN double step_growth(double root_inv, double hi = 6.0, double safety = 0.9) {
  return fmin(hi, fmax(0.2, root_inv * safety));
}

}  // namespace pk
