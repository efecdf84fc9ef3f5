// Host code: eigen decomposition of a small symmetric matrix by cyclic Jacobi in double (pose_inertial.hip: the 15 x 15 of
// Optimizer::Marginalize and of the ConstraintPoseImu constructor, the 9 x 9 / 3 x 3 information matrices).  Not on a hot path.
#pragma once

#include <cmath>

namespace orbg {

// A (n x n, row-major, n <= 16) is read through its LOWER triangle, as Eigen::SelfAdjointEigenSolver does; on return w[k] is an
// eigenvalue (unsorted) and column k of V (row-major n x n) its unit eigenvector.
inline void sym_eig_jacobi(int n, const double* A, double* w, double* V) {
  double a[16 * 16];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      a[i * n + j] = i >= j ? A[i * n + j] : A[j * n + i];
      V[i * n + j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0, dia = 0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) (i == j ? dia : off) += a[i * n + j] * a[i * n + j];
    if (!(off > 1e-36 * dia) || !std::isfinite(off)) break;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = a[p * n + q];
        if (apq == 0.0) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {           // columns p, q
          const double akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - s * akq;
          a[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {           // rows p, q
          const double apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - s * aqk;
          a[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < n; i++) w[i] = a[i * n + i];
}

// out = V diag(f(w)) V^T, all n x n row-major
template <class F>
inline void sym_rebuild(int n, const double* w, const double* V, F f, double* out) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      double s = 0;
      for (int k = 0; k < n; k++) s += V[i * n + k] * f(w[k]) * V[j * n + k];
      out[i * n + j] = s;
    }
}

}  // namespace orbg
