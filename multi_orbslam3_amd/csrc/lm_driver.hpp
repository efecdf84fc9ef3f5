// The host side of g2o's Levenberg-Marquardt as the bundle adjustments run it (lba.hip: Optimizer::LocalBundleAdjustment,
// full_ba.hip: Optimizer::BundleAdjustment): the caller's abort flag with its poll rule, the trace row, and the outer loop of the
// solves that wait for every record (lm_optimize: full_ba.hip, inertial_ba.hip, essential_graph.hip).  The arithmetic of
// OptimizationAlgorithmLevenberg::solve on the three scalars a trial brings back from the device (robust chi2, computeScale, the
// solver's flag) is lm_step.hpp's, where the device's own loops find it too.  What each solve launches around these steps is its own.
#pragma once

#include <cstdint>

#include "lm_step.hpp"

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
