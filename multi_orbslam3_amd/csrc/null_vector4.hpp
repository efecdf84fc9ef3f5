// Null vector of a 4 x 4 homogeneous system A x = 0 as the eigenvector of the smallest eigenvalue of S = A^T A, cyclic Jacobi in
// float64: the project's answer to cv::SVD::compute on a CV_32F 4 x 4 (float32 one-sided Jacobi in OpenCV, not pinned to the bit).
// Used by KannalaBrandt8::Triangulate (matcher.hip) and by the linear triangulation of CreateNewMapPoints (newpoints.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace orbg {

__device__ __forceinline__ void null_vector4(double (&S)[4][4], double (&v)[4]) {   // eigenvector of the smallest eigenvalue of a symmetric 4 x 4: cyclic Jacobi
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0, diag = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      diag += S[p][p] * S[p][p];
#pragma unroll
      for (int q = p + 1; q < 4; q++) off += S[p][q] * S[p][q];
    }
    if (off <= 1e-28 * diag) break;                         // eigenvectors to ~1e-14: far below the float32 the result is rounded to
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        if (S[p][q] == 0.0) continue;
        const double tau = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
#pragma unroll
        for (int k = 0; k < 4; k++) { const double a = S[k][p], b = S[k][q]; S[k][p] = cs * a - sn * b; S[k][q] = sn * a + cs * b; }
#pragma unroll
        for (int k = 0; k < 4; k++) { const double a = S[p][k], b = S[q][k]; S[p][k] = cs * a - sn * b; S[q][k] = sn * a + cs * b; }
#pragma unroll
        for (int k = 0; k < 4; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = cs * a - sn * b; V[k][q] = sn * a + cs * b; }
      }
  }
  int m = 0;
  double smallest = S[0][0];                                // (compile-time indices only: a dynamically indexed array lives in scratch memory)
#pragma unroll
  for (int i = 1; i < 4; i++) if (S[i][i] < smallest) { smallest = S[i][i]; m = i; }
#pragma unroll
  for (int k = 0; k < 4; k++) v[k] = m == 0 ? V[k][0] : m == 1 ? V[k][1] : m == 2 ? V[k][2] : V[k][3];
}

}  // namespace orbg
