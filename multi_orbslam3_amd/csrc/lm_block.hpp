// What the single-workgroup solve kernels share (pose_opt.hip: PoseOptimization, 6 unknowns; sim3_opt.hip: OptimizeSim3, 7;
// pose_inertial.hip: PoseInertialOptimization, 15 / 30; inertial_init.hip: InertialOptimization): the damped solve spread over the lanes
// of a wavefront and the block sum of a 256-thread (four-wavefront) workgroup.  The scalar Huber kernel is lm_step.hpp's, included
// here for all of them; the word that completes a one-launch solve is common.hpp's (SolveWord).
#pragma once

#include "lm_step.hpp"
#include "wave.hpp"

namespace orbg {

// (H + lambda I) x = b by LDL^T without pivoting, spread over lanes 0..N-1 of a wave: lane `li` holds row li.  Every
// subtraction happens in the order of a scalar left-looking factorisation (ascending k), so the factors are the
// same bits a serial solve would produce.  Returns false unless every pivot is positive and finite (Eigen::LDLT::isPositive),
// in which case x is left untouched.  x[] comes out wave-uniform.
// REL (pose_inertial.hip, lambda = 0: Gauss-Newton on a system that can be singular): a pivot no larger than 2^-40 of its own
// diagonal entry has lost every bit but rounding noise to cancellation and counts as not positive -- its sign is arbitrary.
template <int N, bool REL = false>
__device__ inline bool lane_ldlt_solve(const double* Hrow, double b_li, int li, double lambda, double* x) {
  // (round 4, measured and dropped: the seven divisions as products with 1/d from the hardware seed + two Newton steps -- no
  // measurable gain, 162 vs 158-164 us at 450 correspondences, and one of the twelve parity cases changed an iteration count)
  double A[N], D[N];
#pragma unroll
  for (int j = 0; j < N; j++) A[j] = Hrow[j] + (j == li ? lambda : 0.0);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double d = wave_readlane_f64(A[k], k);
    if constexpr (REL) {
      if (!(d > 0x1p-40 * fabs(wave_readlane_f64(Hrow[k], k)))) ok = false;
    }
    if (!(d > 0.0) || fabs(d) == INFINITY) ok = false;
    D[k] = d;
    const double Lik = A[k] / d;
#pragma unroll
    for (int j = k + 1; j < N; j++) { const double Ljk = wave_readlane_f64(Lik, j); A[j] -= (Lik * Ljk) * d; }
    A[k] = Lik;
  }
  if (!ok) return false;
  double y = b_li;
#pragma unroll
  for (int k = 0; k < N - 1; k++) { const double yk = wave_readlane_f64(y, k); if (li > k) y -= A[k] * yk; }
  double Di = D[0];
#pragma unroll
  for (int k = 1; k < N; k++) Di = (li == k) ? D[k] : Di;
  y /= Di;
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    double sv = wave_readlane_f64(y, i);
#pragma unroll
    for (int k = i + 1; k < N; k++) sv -= wave_readlane_f64(A[i], k) * x[k];
    x[i] = sv;
  }
  return true;
}

constexpr int kLmRow = 8 * 33;     // one reduction row: 8 segments of 32 values, padded against LDS bank conflicts

// Block-wide sums of NV per-thread values of a 256-thread workgroup in a fixed order: transpose through LDS (s_acc: NV * kLmRow
// doubles), 8 threads per value add 32 entries each (s_part: NV * 8), one thread per value adds the 8 partials.  out[0..NV) is valid
// for every thread afterwards.
template <int NV>
__device__ inline void lm_block_reduce(const double* vals, double* s_acc, double* s_part, double* out) {
  const int tid = threadIdx.x;
  const int col = (tid >> 5) * 33 + (tid & 31);
#pragma unroll
  for (int v = 0; v < NV; v++) s_acc[v * kLmRow + col] = vals[v];
  __syncthreads();
  if (tid < NV * 8) {
    const double* p = s_acc + (tid >> 3) * kLmRow + (tid & 7) * 33;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { a0 += p[4 * j]; a1 += p[4 * j + 1]; a2 += p[4 * j + 2]; a3 += p[4 * j + 3]; }
    s_part[tid] = (a0 + a1) + (a2 + a3);
  }
  __syncthreads();
  if (tid < NV) {
    const double* p = s_part + tid * 8;
    out[tid] = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
  }
  __syncthreads();
}

// Block-wide sum of ONE double per thread of a four-wavefront workgroup: DPP tree inside each wavefront, the four wave totals through
// LDS, added in wave order by every thread (one barrier; `slot` alternates between consecutive calls so that no second barrier is needed).
__device__ __forceinline__ double block_sum(double v, double (*wsum)[4], int slot) {
  const double w = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) wsum[slot][threadIdx.x >> 6] = w;
  __syncthreads();
  return ((wsum[slot][0] + wsum[slot][1]) + wsum[slot][2]) + wsum[slot][3];
}

}  // namespace orbg
