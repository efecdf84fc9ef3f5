// g2o::Sim3 arithmetic in FP64, shared by OptimizeSim3 (sim3_opt.hip) and OptimizeEssentialGraph (essential_graph.hip): the
// constructor from a 7-vector, operator*, inverse(), map() and log() of G/types/sim3.h.  What Eigen does inside a call is a choice
// made here; the choices E-1 .. E-7 are listed at the top of sim3_opt.hip (tests/sim3_opt_model.py restates them), log() adds
//   E-10 Quaterniond::toRotationMatrix(): se3.hpp quat_to_R (tx = 2 x, twx = tx w, ..., R00 = 1 - (tyy + tzz), R01 = txy - twz, ...).
//   E-11 Matrix3d::lu().solve(): Gaussian elimination with partial pivoting (the row with the largest |entry| of the column, the first
//        one on a tie), L with unit diagonal, forward then backward substitution, every dot product in ascending k.
// Everything is inline and usable on the host too (the solves that need no launch evaluate their chi2 there).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "se3.hpp"

namespace orbg_s3 {

using orbg_se3::quat_from_R;
using orbg_se3::quat_rotate;
using orbg_se3::quat_to_R;

struct S3 { double q[4], t[3], s; };   // g2o::Sim3: rotation().coeffs() (x, y, z, w), translation(), scale()

// Sim3(const Vector7d& update), G/types/sim3.h:70-142, all four branches (E-1, E-4)
__host__ __device__ inline void s3_exp(const double* u, S3* o) {
  const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
  const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
  const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
  const double s = exp(sigma);
  double O2[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
  const double eps = 0.00001;
  double A, B, C, ra = 1.0, rb = 1.0;      // R = I + ra Omega + rb Omega2; the small-angle branches add Omega and Omega2 as they are
  const bool small = theta < eps;
  if (fabs(sigma) < eps) {
    C = 1;
    if (small) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (small) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * sin(theta);
      const double b = s * cos(theta);
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  double R[9];
  if (small) {
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i];
  } else {
    ra = sin(theta) / theta;
    rb = (1 - cos(theta)) / (theta * theta);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ra * O[i] + rb * O2[i];
  }
  quat_from_R(R, o->q);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double W0 = A * O[3 * i] + B * O2[3 * i] + C * (i == 0 ? 1.0 : 0.0);
    const double W1 = A * O[3 * i + 1] + B * O2[3 * i + 1] + C * (i == 1 ? 1.0 : 0.0);
    const double W2 = A * O[3 * i + 2] + B * O2[3 * i + 2] + C * (i == 2 ? 1.0 : 0.0);
    o->t[i] = W0 * u[3] + W1 * u[4] + W2 * u[5];
  }
  o->s = s;
}

// Sim3::operator*, sim3.h:266-272 (E-3, E-7)
__host__ __device__ inline void s3_mul(const S3& a, const S3& b, S3* o) {
  const double* x = a.q; const double* y = b.q;
  o->q[0] = x[3] * y[0] + x[0] * y[3] + x[1] * y[2] - x[2] * y[1];
  o->q[1] = x[3] * y[1] + x[1] * y[3] + x[2] * y[0] - x[0] * y[2];
  o->q[2] = x[3] * y[2] + x[2] * y[3] + x[0] * y[1] - x[1] * y[0];
  o->q[3] = x[3] * y[3] - x[0] * y[0] - x[1] * y[1] - x[2] * y[2];
  double rt[3];
  quat_rotate(a.q, b.t, rt);
#pragma unroll
  for (int i = 0; i < 3; i++) o->t[i] = a.s * rt[i] + a.t[i];
  o->s = a.s * b.s;
}

// Sim3::inverse, sim3.h:233-236 (E-6)
__host__ __device__ inline void s3_inverse(const S3& a, S3* o) {
  o->q[0] = -a.q[0]; o->q[1] = -a.q[1]; o->q[2] = -a.q[2]; o->q[3] = a.q[3];
  const double k = -1. / a.s;
  const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
  quat_rotate(o->q, v, o->t);
  o->s = 1. / a.s;
}

// Sim3::map, sim3.h:144-146 (E-6): s * (r * xyz) + t
__host__ __device__ inline void s3_map(const S3& a, const double* X, double* out) {
  double r[3];
  quat_rotate(a.q, X, r);
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = a.s * r[i] + a.t[i];
}

// Sim3::log, sim3.h:148-230, all four branches (E-4, E-10, E-11); deltaR and skew: G/types/se3_ops.hpp
__host__ __device__ inline void s3_log(const S3& a, double* res) {
  const double s = a.s;
  const double sigma = log(s);
  double R[9];
  quat_to_R(a.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double eps = 0.00001;
  double A, B, C, k;
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      k = 0.5;
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta = acos(d);
      const double theta2 = theta * theta;
      k = theta / (2 * sqrt(1 - d * d));
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      k = 0.5;
      A = ((sigma - 1) * s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      k = theta / (2 * sqrt(1 - d * d));
      const double theta2 = theta * theta;
      const double sa = s * sin(theta);
      const double sb = s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (sa * sigma + (1 - sb) * theta) / (theta * c);
      B = (C - ((sb - 1) * sigma + sa * theta) / (c)) * 1. / (theta2);
    }
  }
  const double om0 = k * dR[0], om1 = k * dR[1], om2 = k * dR[2];
  const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
  // W = A Omega + B Omega Omega + C I, rows r0 r1 r2 with the right-hand side as a fourth column
  double r0[4], r1[4], r2[4];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    r0[j] = A * O[j] + B * (O[0] * O[j] + O[1] * O[3 + j] + O[2] * O[6 + j]) + C * (j == 0 ? 1.0 : 0.0);
    r1[j] = A * O[3 + j] + B * (O[3] * O[j] + O[4] * O[3 + j] + O[5] * O[6 + j]) + C * (j == 1 ? 1.0 : 0.0);
    r2[j] = A * O[6 + j] + B * (O[6] * O[j] + O[7] * O[3 + j] + O[8] * O[6 + j]) + C * (j == 2 ? 1.0 : 0.0);
  }
  r0[3] = a.t[0]; r1[3] = a.t[1]; r2[3] = a.t[2];
  // partial-pivot elimination; rows are swapped by value so that no local array is indexed at run time
#define ORBG_S3_SWAP(x, y) { _Pragma("unroll") for (int j = 0; j < 4; j++) { const double tmp = x[j]; x[j] = y[j]; y[j] = tmp; } }
  {
    const double a0 = fabs(r0[0]), a1 = fabs(r1[0]), a2 = fabs(r2[0]);
    if (a1 > a0 && a1 >= a2) ORBG_S3_SWAP(r0, r1)
    else if (a2 > a0 && a2 > a1) ORBG_S3_SWAP(r0, r2)
  }
  const double l10 = r1[0] / r0[0], l20 = r2[0] / r0[0];
  r1[1] -= l10 * r0[1]; r1[2] -= l10 * r0[2];
  r2[1] -= l20 * r0[1]; r2[2] -= l20 * r0[2];
  double y0 = r0[3], y1 = r1[3], y2 = r2[3];
  double m10 = l10, m20 = l20;
  if (fabs(r2[1]) > fabs(r1[1])) {
    ORBG_S3_SWAP(r1, r2)
    { const double tmp = y1; y1 = y2; y2 = tmp; }
    { const double tmp = m10; m10 = m20; m20 = tmp; }
  }
#undef ORBG_S3_SWAP
  const double l21 = r2[1] / r1[1];
  const double u22 = r2[2] - l21 * r1[2];
  // L y = P t, then U upsilon = y
  y1 = y1 - m10 * y0;
  y2 = y2 - m20 * y0 - l21 * y1;
  const double x2 = y2 / u22;
  const double x1 = (y1 - r1[2] * x2) / r1[1];
  const double x0 = (y0 - r0[1] * x1 - r0[2] * x2) / r0[0];
  res[0] = om0; res[1] = om1; res[2] = om2;
  res[3] = x0; res[4] = x1; res[5] = x2;
  res[6] = sigma;
}

}  // namespace orbg_s3
