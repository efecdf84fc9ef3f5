// The record an LM solve that waits for every verdict (lm_optimize, lm_driver.hpp: full_ba.hip, inertial_ba.hip, essential_graph.hip)
// reads back after a linearisation or a trial, the one-workgroup reduction that writes it, and the host's way to it.  What the host
// decides from a record is lm_step.hpp's (lm_trial_verdict, lm_lambda_init on .maxdiag).  Every sum has a
// fixed order: two calls on the same input return the same bits.
#pragma once

#include "common.hpp"
#include "wave.hpp"

namespace orbg_lm {

// robust chi2 of the evaluation, computeScale's sum and the solver's flag (a trial's), the largest diagonal entry (a linearisation's)
struct LmRec { double chi2, scale, maxdiag; int ok, pad; };

// sum of v over the workgroup (256 threads) in a fixed order, valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* red /* 4 */) {
  const double w = orbg::wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup of 256 threads: the sums of the partials and of the scale terms in index order (thread t sums a contiguous chunk in
// order, the 256 chunk sums go through the fixed tree), the largest of the threads' diagonal candidates `m`, the solver's flag (none:
// 1) -> the record.  A solve whose lambda never comes from the diagonal (kMaxDiag false) skips the max tree: maxdiag = 0.
template <bool kMaxDiag = true>
__device__ __forceinline__ void lm_finish_record(int n_partial, const double* __restrict__ partial, int n_scale, const double* __restrict__ scale_v,
                                                 double m, const int* __restrict__ ok_flag, LmRec* __restrict__ rec) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double s = 0;
  { const int ch = (n_partial + 255) / 256; const int b = min(n_partial, tid * ch), e = min(n_partial, b + ch); for (int i = b; i < e; i++) s += partial[i]; }
  const double chi = block_sum_256(s, red);
  s = 0;
  { const int ch = (n_scale + 255) / 256; const int b = min(n_scale, tid * ch), e = min(n_scale, b + ch); for (int i = b; i < e; i++) s += scale_v[i]; }
  const double scale = block_sum_256(s, red);
  double maxdiag = 0;
  if constexpr (kMaxDiag) {
    __shared__ double mx[256];
    mx[tid] = m;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) { if (tid < s2) mx[tid] = fmax(mx[tid], mx[tid + s2]); __syncthreads(); }
    maxdiag = mx[0];
  }
  if (tid == 0) { rec->chi2 = chi; rec->scale = scale; rec->maxdiag = maxdiag; rec->ok = ok_flag ? *ok_flag : 1; }
}

// the record of the last launches, on the host: the wait of a linearisation or a trial, where the phase timer reads its events
template <class Timer>
int lm_fetch_record(LmRec* host, const LmRec* dev, hipStream_t st, Timer& timer) {
  ORBG_HIP(hipGetLastError());
  ORBG_HIP(hipMemcpyAsync(host, dev, sizeof(LmRec), hipMemcpyDeviceToHost, st));
  ORBG_HIP(hipStreamSynchronize(st));
  timer.flush(st);
  return ORBG_OK;
}

}  // namespace orbg_lm
