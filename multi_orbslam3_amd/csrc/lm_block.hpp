// What the single-workgroup Levenberg-Marquardt kernels share (pose_opt.hip: PoseOptimization, 6 unknowns; sim3_opt.hip: OptimizeSim3,
// 7): the damped solve spread over the lanes of a wavefront and the block sum of a 256-thread (four-wavefront) workgroup.
#pragma once

#include "wave.hpp"

namespace orbg {

// (H + lambda I) x = b by LDL^T without pivoting, spread over lanes 0..N-1 of a wave: lane `li` holds row li.  Every
// subtraction happens in the order of a scalar left-looking factorisation (ascending k), so the factors are the
// same bits a serial solve would produce.  Returns false unless every pivot is positive and finite (Eigen::LDLT::isPositive),
// in which case x is left untouched.  x[] comes out wave-uniform.
template <int N>
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

// Block-wide sum of ONE double per thread of a four-wavefront workgroup: DPP tree inside each wavefront, the four wave totals through
// LDS, added in wave order by every thread (one barrier; `slot` alternates between consecutive calls so that no second barrier is needed).
__device__ __forceinline__ double block_sum(double v, double (*wsum)[4], int slot) {
  const double w = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) wsum[slot][threadIdx.x >> 6] = w;
  __syncthreads();
  return ((wsum[slot][0] + wsum[slot][1]) + wsum[slot][2]) + wsum[slot][3];
}

}  // namespace orbg
