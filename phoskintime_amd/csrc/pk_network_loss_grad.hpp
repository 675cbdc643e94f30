// pk_network_loss_grad.hpp -- derivatives of the network loss's two scalar building blocks: the eight LOSS_MODE point losses with respect to
// the prediction, and the floored fold change of LOSS_FN with respect to numerator and baseline.  The values themselves stay where they
// are (point_loss / fold_change, pk_network.hpp); this header restates only what their derivatives need.  Plain C++ over <math.h>: device
// code under hipcc (the scoring flavour of net_rosw_sens_solve, pk_network_sens.hpp), host code under g++
// (tests/test_net_loss_grad_cpu.py).  No statics, no HIP headers in the host build.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PK_LG_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PK_LG_FN inline
#endif

namespace pk {

constexpr double kLossFloor = 1e-9;       // EPS of LOSS_FN (lossfn.py:24): floor of the fold change, shift inside the logs of mode 2

// d/d pred of point_loss(mode, obs - pred, obs, pred).  With diff = obs - pred every mode but 5 depends on pred through diff alone, so the
// result is -rho'(diff); mode 5 also divides by |pred| + 1e-6.  At a kink the derivative is that of the branch the value takes (mode 1:
// the quadratic at |diff| = 0.5; mode 3: log cosh at |diff| = 20).  Mode 2 is NaN where its value is NaN (diff + 1e-9 < 0)
PK_LG_FN double point_loss_dpred(const int mode, const double obs, const double pred) {
  const double diff = obs - pred;
  switch (mode) {
    case 0: return -2.0 * diff;
    case 1: { const double a = fabs(diff), d = 0.5; return a <= d ? -diff : (diff > 0.0 ? -d : d); }
    case 2: {
      const double sh = diff + kLossFloor;
      const double x = (log(sh) - log(obs + kLossFloor)) / 0.5;
      return -(0.5 * x) / (sqrt(1.0 + x * x) * sh);
    }
    case 3: { const double s = fabs(diff); return s > 20.0 ? (diff > 0.0 ? -1.0 : 1.0) : -tanh(diff); }
    case 4: return -(2.0 * diff) / (1.0 + diff * diff);
    case 5: {
      const double q = fabs(pred) + 1e-6;
      const double sg = pred > 0.0 ? 1.0 : (pred < 0.0 ? -1.0 : 0.0);
      return -(2.0 * diff) / q - sg * ((diff * diff) / (q * q));
    }
    case 6: { const double q = diff * diff + 1.0; return -(2.0 * diff) / (q * q); }
    default: return -diff / sqrt(diff * diff + 1e-3 * 1e-3);
  }
}

// Tangent of the floored fold change p = max(a, eps) / max(c, eps) along (da, dc): dp = [a > eps] da / c_m - p [c > eps] dc / c_m with
// c_m = max(c, eps); the derivative through an active floor is 0.  p is formed as fold_change forms it
PK_LG_FN double fold_change_tangent(const double a, const double c, const double da, const double dc) {
  const double am = a > kLossFloor ? a : kLossFloor, cm = c > kLossFloor ? c : kLossFloor;
  const double p = am / cm;
  const double ta = a > kLossFloor ? da : 0.0, tc = c > kLossFloor ? dc : 0.0;
  return (ta - p * tc) / cm;
}

}  // namespace pk
