// The host side of g2o's Levenberg-Marquardt as the bundle adjustments run it (lba.hip: Optimizer::LocalBundleAdjustment,
// full_ba.hip: Optimizer::BundleAdjustment): the caller's abort flag with its poll rule, and the arithmetic of
// OptimizationAlgorithmLevenberg::solve on the three scalars a trial brings back from the device (robust chi2, computeScale, the
// solver's flag).  What each solve launches around these steps is its own; the decisions are written once, here, and so is the
// outer loop of the solves that wait for every record (lm_optimize: full_ba.hip, essential_graph.hip).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

namespace orbg_lm {

// The abort flag as the caller owns it: the C-ABI's int32 (with its deterministic test forms) or the reference's own
// one-byte bool (LocalMapping::mbAbortBA behind Optimizer::LocalBundleAdjustment's bool* pbStopFlag, S/LocalMapping.cc:381-386;
// LoopClosing::mbStopGBA behind Optimizer::GlobalBundleAdjustemnt's, S/LoopClosing.cc:2627)
struct StopRef {
  const volatile int32_t* i32 = nullptr;
  const volatile uint8_t* u8 = nullptr;
};

// g2o's termination test: > 0 stops (the reference's bool); < 0 stops once that many LM trials have been evaluated (deterministic
// test hook, orbgpu.h); INT32_MIN is raised right after the check that precedes optimize() (the -k form with k = 0)
struct StopCheck {
  StopRef ref;
  int trials_done = 0;
  bool past_precheck = false;
  bool operator()() const {
    if (ref.u8) return *ref.u8 != 0;
    if (!ref.i32) return false;
    const int v = *ref.i32;
    if (v == INT32_MIN) return past_precheck;
    return v > 0 || (v < 0 && trials_done >= -v);
  }
};

// lambda, the rejection factor, the chi2 of the current estimate and the count of iterations that barely improved it
struct LmScalars {
  double lambda = -1, ni = 2, currentChi = 0;
  int nBad = 0;
};

// computeLambdaInit (G/core/optimization_algorithm_levenberg.cpp:161-174): the user's value, or tau * the largest diagonal entry
inline double lm_lambda_init(double user_lambda, double max_diagonal) { return user_lambda > 0 ? user_lambda : 1e-5 * max_diagonal; }

// The verdict on one trial (G/core/optimization_algorithm_levenberg.cpp:118-146): rho = (chi2 - chi2_trial) / (scale + 1e-3).
// Accepted (rho > 0 and a finite chi2_trial): lambda shrinks by max(1/3, min(1 - (2 rho - 1)^3, 2/3)) and the trial's chi2 becomes
// the current one; rejected: lambda *= ni, ni *= 2.  Returns rho.
inline double lm_trial_verdict(LmScalars& m, bool solver_ok, double chi2_trial, double scale, bool* accepted) {
  double tempChi = chi2_trial;
  if (!solver_ok) tempChi = std::numeric_limits<double>::max();
  double rho = m.currentChi - tempChi;
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && std::isfinite(tempChi)) {
    const double c3 = 2 * rho - 1;               // (2 rho - 1)^3 as two multiplications: lba.hip's publish_trial_record does the same
    double alpha = 1. - c3 * c3 * c3;            // arithmetic on the device for the speculative next solve
    alpha = std::min(alpha, 2. / 3.);
    const double scaleFactor = std::max(1. / 3., alpha);
    m.lambda *= scaleFactor;
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
inline bool lm_try_again(double rho, bool trials_left, bool stop_raised) { return rho < 0 && trials_left && !stop_raised; }

// The end of an iteration: false when optimize() ends with it -- the trials ran out (the caller's qmax == maxTrialsAfterFailure), a
// trial with rho == 0, or the third iteration in a row that improved chi2 by less than a thousandth.
inline bool lm_iteration_continues(LmScalars& m, bool trials_exhausted, double rho, double iniChi) {
  if (trials_exhausted || rho == 0) return false;
  if ((iniChi - m.currentChi) * 1e3 < iniChi) m.nBad++; else m.nBad = 0;
  return m.nBad < 3;
}

// the trace row of an iteration as the bundle adjustments report it: lambda, the chi2 reached, the trials it took
inline void lm_trace_row(const LmScalars& m, int qmax, double* trace, int cap, int* len) {
  if (!trace || *len >= cap) return;
  double* t = trace + 3 * (size_t)*len;
  t[0] = m.lambda; t[1] = m.currentChi; t[2] = qmax;
  ++*len;
}

// SparseOptimizer::optimize with OptimizationAlgorithmLevenberg::solve as its iteration, for the solves that wait for every record
// (full_ba.hip, essential_graph.hip; the local BA launches ahead of its verdicts and keeps a loop of its own).  Run supplies:
//   LmScalars lm
//   int linearise()                          computeActiveErrors + buildSystem of the current estimate; 0 or the code to leave with
//   int trial(double lambda)                 solve, the trial state, its evaluation; likewise
//   record()                                 of the last of those launches: .chi2, .maxdiag (a linearisation's), .scale, .ok (a trial's)
//   int timed_out()                          the code to leave with when that .ok is no verdict on the system, else 0
//   void accept()                            discardTop(): the trial state becomes the current one (pop() otherwise: nothing to do)
//   int first_linearisation(double* lambda)  what the solve keeps of iteration 0's record; *lambda = the user's lambda (<= 0: none)
//   void iteration_done(int qmax, bool accepted)   the iteration's trace row, the chi2 reached
// `stop` counts the evaluated trials (a solve without an abort flag passes a StopCheck without one); *done = iterations run.
template <class Run>
int lm_optimize(Run& run, int iterations, StopCheck& stop, int* done) {
  LmScalars& lm = run.lm;
  int rc;
  bool ok = true;
  *done = 0;
  for (int it = 0; it < iterations && !stop() && ok; it++) {
    if ((rc = run.linearise())) return rc;
    lm.currentChi = run.record().chi2;
    if (it == 0) {
      double user_lambda = 0;
      if ((rc = run.first_linearisation(&user_lambda))) return rc;
      lm.lambda = lm_lambda_init(user_lambda, run.record().maxdiag);
      lm.ni = 2; lm.nBad = 0;
    }
    const double iniChi = lm.currentChi;
    double rho = 0;
    int qmax = 0;
    bool accepted = false;
    do {
      if ((rc = run.trial(lm.lambda)) || (rc = run.timed_out())) return rc;
      rho = lm_trial_verdict(lm, run.record().ok != 0, run.record().chi2, run.record().scale, &accepted);
      if (accepted) run.accept();
      qmax++;
      stop.trials_done++;
    } while (lm_try_again(rho, qmax < 10, stop()));
    ++*done;
    run.iteration_done(qmax, accepted);
    ok = lm_iteration_continues(lm, qmax == 10, rho, iniChi);
  }
  return 0;
}

}  // namespace orbg_lm
