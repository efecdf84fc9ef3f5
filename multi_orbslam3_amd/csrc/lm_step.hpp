// The decisions of one step of g2o's Levenberg-Marquardt (OptimizationAlgorithmLevenberg::solve) and the scalar Huber kernel, written
// once for the host and the device: the bundle adjustments' host loops (lm_driver.hpp, lba.hip) and the local BA's speculative lambda
// on the device (lba.hip: publish_trial_tail) run these lines, every edge kernel of the bundle adjustments and of the inertial
// optimisers its Huber kernel.  (The one-launch LM kernels -- pose_opt.hip, sim3_opt.hip, inertial_init.hip -- keep their own written-out
// step: with calls to these functions they measured 0.5 - 1.5 % slower, docs/experiments.md.)  Nothing here calls into std:: -- only + - * / sqrt, compares and min / max -- so both sides produce the same bits
// (tools/micro/device_math_test.hip runs every function in both modes).
#pragma once

#include <math.h>

#define LM_HD __host__ __device__ __forceinline__      // (every unit that includes this header is compiled as HIP)

namespace orbg_lm {

// _goodStepLowerScale, _goodStepUpperScale (G/core/optimization_algorithm_levenberg.cpp:47-51)
constexpr double kLmGoodStepLower = 1. / 3., kLmGoodStepUpper = 2. / 3.;

// lambda, the rejection factor, the chi2 of the current estimate and the count of iterations that barely improved it
struct LmScalars {
  double lambda = -1, ni = 2, currentChi = 0;
  int nBad = 0;
};

// computeLambdaInit (G/core/optimization_algorithm_levenberg.cpp:161-174): the user's value, or tau * the largest diagonal entry.  (How
// the largest entry is found stays with each solve: the two forms in use differ on a NaN diagonal.)
LM_HD double lm_lambda_init(double user_lambda, double max_diagonal) { return user_lambda > 0 ? user_lambda : 1e-5 * max_diagonal; }

// lambda after an accepted trial (:126-131): lambda * max(1/3, min(1 - (2 rho - 1)^3, 2/3)), the cube as two multiplications.  Reached
// with rho > 0 only, where alpha is finite or -inf: min / max never see a NaN.
LM_HD double lm_accepted_lambda(double lambda, double rho) {
  const double c3 = 2 * rho - 1;
  double alpha = 1. - c3 * c3 * c3;
  alpha = fmin(alpha, kLmGoodStepUpper);
  return lambda * fmax(kLmGoodStepLower, alpha);
}

// what a refused solve counts as (:118-121: std::numeric_limits<double>::max(), not infinity)
LM_HD double lm_trial_chi2(bool solver_ok, double chi2_trial) { return solver_ok ? chi2_trial : 1.7976931348623157e308; }

// The verdict on one trial (:118-146): rho = (chi2 - chi2_trial) / (scale + 1e-3).  Accepted (rho > 0 and a finite chi2_trial): lambda
// shrinks (lm_accepted_lambda) and the trial's chi2 becomes the current one; rejected: lambda *= ni, ni *= 2.  Returns rho.
LM_HD double lm_trial_verdict(LmScalars& m, bool solver_ok, double chi2_trial, double scale, bool* accepted) {
  const double tempChi = lm_trial_chi2(solver_ok, chi2_trial);
  double rho = m.currentChi - tempChi;
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && fabs(tempChi) != INFINITY && tempChi == tempChi) {      // g2o_isfinite(tempChi)
    m.lambda = lm_accepted_lambda(m.lambda, rho);
    m.ni = 2;
    m.currentChi = tempChi;
    *accepted = true;
  } else {
    m.lambda *= m.ni;
    m.ni *= 2;
    *accepted = false;
  }
  return rho;
}
// the trial loop goes on while the last trial was rejected with rho < 0, trials are left (the caller's qmax < maxTrialsAfterFailure:
// g2o's property, 10 in every solve of the reference) and the flag is down
LM_HD bool lm_try_again(double rho, bool trials_left, bool stop_raised) { return rho < 0 && trials_left && !stop_raised; }

// The end of an iteration: false when optimize() ends with it -- the trials ran out (the caller's qmax == maxTrialsAfterFailure), a
// trial with rho == 0, or the third iteration in a row that improved chi2 by less than a thousandth.
LM_HD bool lm_iteration_continues(LmScalars& m, bool trials_exhausted, double rho, double iniChi) {
  if (trials_exhausted || rho == 0) return false;
  if ((iniChi - m.currentChi) * 1e3 < iniChi) m.nBad++; else m.nBad = 0;
  return m.nBad < 3;
}

// rho[0], rho[1] of RobustKernelHuber::robustify (G/core/robust_kernel_impl.cpp:78-91); a NaN e takes the else branch, as there
LM_HD void lm_huber(double e, double delta, double dsqr, double* rho0, double* rho1) {
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
  else { const double s = sqrt(e); *rho0 = 2 * s * delta - dsqr; *rho1 = delta / s; }
}

}  // namespace orbg_lm
