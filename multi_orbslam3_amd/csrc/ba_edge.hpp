// The reprojection edges of the bundle adjustments (lba.hip: Optimizer::LocalBundleAdjustment, full_ba.hip:
// Optimizer::BundleAdjustment): residual, depth test, Huber thresholds (the kernel itself is lm_step.hpp's lm_huber) and the
// analytic Jacobians of one edge.  No include guard and no namespace of its own: each translation unit includes it ONCE inside its
// anonymous namespace, after se3.hpp and `using namespace orbg_se3`, so that each unit keeps its own internal copies.

__device__ inline void edge_error(const PoseQ& T, const double* X, const Cam& c, const lba_edge& e, double* err, double* Xc) {
  double r[3];
  quat_rotate(T.q, X, r);
  Xc[0] = r[0] + T.t[0]; Xc[1] = r[1] + T.t[1]; Xc[2] = r[2] + T.t[2];
  if (e.ur < 0) {
    const double iz = 1.0 / Xc[2];
    err[0] = (double)e.u - (c.fx * Xc[0] * iz + c.cx);
    err[1] = (double)e.v - (c.fy * Xc[1] * iz + c.cy);
    err[2] = 0;
  } else {
    const float invz = (float)(1.0 / Xc[2]);                 // cam_project: float invz (types_six_dof_expmap.cpp:191)
    const double r0 = Xc[0] * invz * c.fx + c.cx;
    const double r1 = Xc[1] * invz * c.fy + c.cy;
    const double r2 = r0 - (double)(c.bf_f * invz);
    err[0] = (double)e.u - r0; err[1] = (double)e.v - r1; err[2] = (double)e.ur - r2;
  }
}

// The same for a problem that carries an orbg_camera_rig: stereo edges as above; monocular edges through mpCamera->project
// (EdgeSE3ProjectXYZ::computeError, I/OptimizableTypes.h:99-104); the right camera's through mpCamera2 after (mTrl * T)
// (EdgeSE3ProjectXYZToBody::computeError, :127-132).  Xc: the point in the frame of the camera that made the observation.
__device__ inline void edge_error(const PoseQ& T, const double* X, const CamRig& g, const lba_edge& e, double* err, double* Xc) {
  if (e.ur >= 0) { edge_error(T, X, g.c, e, err, Xc); return; }
  double r[3], uv[2];
  if (g.has_right && ur_is_right(e.ur)) {
    PoseQ Trw;
    se3_mul(g.Trl, T, &Trw);
    quat_rotate(Trw.q, X, r);
    Xc[0] = r[0] + Trw.t[0]; Xc[1] = r[1] + Trw.t[1]; Xc[2] = r[2] + Trw.t[2];
    cam_project(g.right, Xc, uv);
  } else {
    quat_rotate(T.q, X, r);
    Xc[0] = r[0] + T.t[0]; Xc[1] = r[1] + T.t[1]; Xc[2] = r[2] + T.t[2];
    cam_project(g.left, Xc, uv);
  }
  err[0] = (double)e.u - uv[0]; err[1] = (double)e.v - uv[1]; err[2] = 0;
}

// isDepthPositive() of an edge: z of the point in the observing camera's frame (G/types/types_six_dof_expmap.h:163-167,
// I/OptimizableTypes.h:106-110,134-138)
__device__ inline bool edge_depth_positive(const PoseQ& T, const double* X, const Cam&, const lba_edge&) {
  double rr[3];
  quat_rotate(T.q, X, rr);
  return rr[2] + T.t[2] > 0.0;
}
__device__ inline bool edge_depth_positive(const PoseQ& T, const double* X, const CamRig& g, const lba_edge& e) {
  double rr[3];
  if (g.has_right && ur_is_right(e.ur)) {
    PoseQ Trw;
    se3_mul(g.Trl, T, &Trw);
    quat_rotate(Trw.q, X, rr);
    return rr[2] + Trw.t[2] > 0.0;
  }
  quat_rotate(T.q, X, rr);
  return rr[2] + T.t[2] > 0.0;
}

// the thresholds of the two edge kinds for lm_huber (lm_step.hpp)
struct Huber { double delta_mono, dsqr_mono, delta_stereo, dsqr_stereo; };

// Jacobians of one edge (stereo: G/types/types_six_dof_expmap.cpp:228-274; mono: S/OptimizableTypes.cpp:139-160)
__device__ inline void edge_jacobians(const PoseQ& T, double x, double y, double z, const Cam& c, float ur, double* A, double* B) {
  const bool mono = ur < 0;
  double R[9];
  quat_to_R(T.q, R);
  const double iz = 1.0 / z, iz2 = iz * iz;     // one division per edge; the reference divides term by term (<= 2 ulp apart)
  if (mono) {
    const double J[6] = {-(c.fx * iz), -0.0, c.fx * x * iz2, -0.0, -(c.fy * iz), c.fy * y * iz2};
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) A[3 * i + j] = J[3 * i] * R[j] + J[3 * i + 1] * R[3 + j] + J[3 * i + 2] * R[6 + j];
    const double S[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) B[6 * i + j] = J[3 * i] * S[j] + J[3 * i + 1] * S[6 + j] + J[3 * i + 2] * S[12 + j];
#pragma unroll
    for (int j = 0; j < 3; j++) A[6 + j] = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) B[12 + j] = 0;
  } else {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      A[j] = -c.fx * R[j] * iz + c.fx * x * R[6 + j] * iz2;
      A[3 + j] = -c.fy * R[3 + j] * iz + c.fy * y * R[6 + j] * iz2;
      A[6 + j] = A[j] - c.bf * R[6 + j] * iz2;
    }
    B[0] = x * y * iz2 * c.fx; B[1] = -(1 + (x * x * iz2)) * c.fx; B[2] = y * iz * c.fx; B[3] = -iz * c.fx; B[4] = 0; B[5] = x * iz2 * c.fx;
    B[6] = (1 + y * y * iz2) * c.fy; B[7] = -x * y * iz2 * c.fy; B[8] = -x * iz * c.fy; B[9] = 0; B[10] = -iz * c.fy; B[11] = y * iz2 * c.fy;
    B[12] = B[0] - c.bf * y * iz2; B[13] = B[1] + c.bf * x * iz2; B[14] = B[2]; B[15] = B[3]; B[16] = 0; B[17] = B[5] - c.bf * iz2;
  }
}

// With a camera rig: (x, y, z) = T.map(X) is the point in the LEFT camera's (body) frame for every kind of edge.
//   monocular  S/OptimizableTypes.cpp:139-160   Xi = -projectJac(X_l) * R(T),                  Xj = -projectJac(X_l) * SE3deriv(X_l)
//   right cam  S/OptimizableTypes.cpp:192-214   Xi = -projectJac(X_r) * R(mTrl * T),  Xj = -projectJac(X_r) * R(mTrl) * SE3deriv(X_l),
//              X_r = mTrl.map(X_l)
__device__ inline void edge_jacobians(const PoseQ& T, double x, double y, double z, const CamRig& g, float ur, double* A, double* B) {
  if (ur >= 0) { edge_jacobians(T, x, y, z, g.c, ur, A, B); return; }
  const double Xl[3] = {x, y, z};
  double R[9], J[6], M[6];
  if (g.has_right && ur_is_right(ur)) {
    double rr[3], Xr[3], Rrl[9];
    quat_rotate(g.Trl.q, Xl, rr);
    Xr[0] = rr[0] + g.Trl.t[0]; Xr[1] = rr[1] + g.Trl.t[1]; Xr[2] = rr[2] + g.Trl.t[2];
    cam_project_jac(g.right, Xr, J);
#pragma unroll
    for (int i = 0; i < 6; i++) J[i] = -J[i];
    PoseQ Trw;
    se3_mul(g.Trl, T, &Trw);
    quat_to_R(Trw.q, R);
    quat_to_R(g.Trl.q, Rrl);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) M[3 * i + j] = J[3 * i] * Rrl[j] + J[3 * i + 1] * Rrl[3 + j] + J[3 * i + 2] * Rrl[6 + j];
  } else {
    cam_project_jac(g.left, Xl, J);
#pragma unroll
    for (int i = 0; i < 6; i++) { J[i] = -J[i]; M[i] = J[i]; }
    quat_to_R(T.q, R);
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) A[3 * i + j] = J[3 * i] * R[j] + J[3 * i + 1] * R[3 + j] + J[3 * i + 2] * R[6 + j];
  const double S[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) B[6 * i + j] = M[3 * i] * S[j] + M[3 * i + 1] * S[6 + j] + M[3 * i + 2] * S[12 + j];
#pragma unroll
  for (int j = 0; j < 3; j++) A[6 + j] = 0;
#pragma unroll
  for (int j = 0; j < 6; j++) B[12 + j] = 0;
}
