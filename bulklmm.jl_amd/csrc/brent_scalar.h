// brent_scalar.h -- Optim.jl's Brent() on the gridbrent sub-intervals (src/gridbrent.jl:9-24; oracle/bulklmm_oracle.py:brent_optim)
// for searches in which every thread of the group evaluates the same scalar sequence: kernels_dyn.hip (run-time covariate counts)
// and kernels_cond.hip (per-trait null designs).  kernels_prep.hip's brent_search is the per-lane form of the same iteration.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace blmm {

template <typename F>
__device__ __forceinline__ double dyn_brent_search(F& f, int nint, int* hit_max) {
  const double golden = 0.5 * (3.0 - sqrt(5.0));
  const double rel_tol = 1.4901161193847656e-08, abs_tol = 2.220446049250313e-16;
  double best_x = 0.0, best_f = INFINITY;
  for (int iv = 0; iv < nint; ++iv) {
    double x_lower = (double)iv / (double)nint, x_upper = (iv + 1 == nint) ? 1.0 : (double)(iv + 1) / (double)nint;
    double new_minimizer = x_lower + golden * (x_upper - x_lower);
    double new_minimum = f(new_minimizer);
    double step = 0.0, old_step = 0.0;
    double old_minimizer = new_minimizer, old_old_minimizer = new_minimizer;
    double old_minimum = new_minimum, old_old_minimum = new_minimum;
    bool done = false;
    int it = 0;
    for (; it < 1000; ++it) {
      double p = 0.0, q = 0.0;
      const double x_tol = rel_tol * fabs(new_minimizer) + abs_tol;
      const double x_mid = (x_upper + x_lower) / 2;
      if (fabs(new_minimizer - x_mid) <= 2 * x_tol - (x_upper - x_lower) / 2) { done = true; break; }
      if (fabs(old_step) > x_tol) {
        const double r = (new_minimizer - old_minimizer) * (new_minimum - old_old_minimum);
        q = (new_minimizer - old_old_minimizer) * (new_minimum - old_minimum);
        p = (new_minimizer - old_old_minimizer) * q - (new_minimizer - old_minimizer) * r;
        q = 2 * (q - r);
        if (q > 0) p = -p; else q = -q;
      }
      double nstep, nold;
      if (fabs(p) < fabs(q * old_step / 2) && p < q * (x_upper - new_minimizer) && p < q * (new_minimizer - x_lower)) {
        nold = step;
        nstep = p / q;
        const double x_temp = new_minimizer + nstep;
        if ((x_temp - x_lower) < 2 * x_tol || (x_upper - x_temp) < 2 * x_tol) nstep = (new_minimizer < x_mid) ? x_tol : -x_tol;
      } else {
        nold = (new_minimizer < x_mid) ? x_upper - new_minimizer : x_lower - new_minimizer;
        nstep = golden * nold;
      }
      const double new_x = (fabs(nstep) >= x_tol) ? new_minimizer + nstep : new_minimizer + ((nstep > 0) ? x_tol : -x_tol);
      const double new_f = f(new_x);
      old_step = nold; step = nstep;
      if (new_f < new_minimum) {
        if (new_x < new_minimizer) x_upper = new_minimizer; else x_lower = new_minimizer;
        old_old_minimizer = old_minimizer; old_old_minimum = old_minimum;
        old_minimizer = new_minimizer; old_minimum = new_minimum;
        new_minimizer = new_x; new_minimum = new_f;
      } else {
        if (new_x < new_minimizer) x_lower = new_x; else x_upper = new_x;
        if (new_f <= old_minimum || old_minimizer == new_minimizer) {
          old_old_minimizer = old_minimizer; old_old_minimum = old_minimum;
          old_minimizer = new_x; old_minimum = new_f;
        } else if (new_f <= old_old_minimum || old_old_minimizer == new_minimizer || old_old_minimizer == old_minimizer) {
          old_old_minimizer = new_x; old_old_minimum = new_f;
        }
      }
    }
    if (it >= 1000 && !done) *hit_max = 1;
    if (new_minimum < best_f || iv == 0) { best_f = new_minimum; best_x = new_minimizer; }
  }
  return best_x;
}

}  // namespace blmm
