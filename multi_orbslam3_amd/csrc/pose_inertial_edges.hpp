// The vertices and edges of an inertial agent's optimisers, for the device and for the host: ImuCamPose and its update, the SO3 functions,
// EdgeInertial, EdgeGyroRW / EdgeAccRW, EdgePriorPoseImu and the pose-only visual edges (S/G2oTypes.cc, I/G2oTypes.h), all in double.
// Shared by pose_inertial.hip (PoseInertialOptimization) and inertial_ba.hip (LocalInertialBA).  No include guard and no namespace of
// its own: each translation unit includes it ONCE inside its anonymous namespace.

constexpr int kPiLd = 32;            // row stride of the stacked matrices: up to 30 unknowns + the error column

struct PiState { double R[9], t[3], v[3], bg[3], ba[3]; };
// everything the kernel reads besides the per-correspondence arrays, widened to double by the host
struct PiParams {
  int n, form, rec_init, pad;
  double fx, fy, cx, cy, bf;
  double Rcb[9], tcb[3];
  PiState cur, oth;
  double dT, dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], lbg[3], lba[3];
  double info9[81], infoG[9], infoA[9];
  PiState prior;
  double priorH[225];
};

// The edge arithmetic below also compiles for the host: pose_inertial_host_linearize runs it without a device, against the numpy model.
#define PI_HD __host__ __device__

// ---- 3 x 3 helpers (row-major)
PI_HD __forceinline__ void m3_mul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
PI_HD __forceinline__ void m3_tmul(const double* A, const double* B, double* C) {     // A^T B
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
PI_HD __forceinline__ void m3_mult(const double* A, const double* B, double* C) {     // A B^T
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
PI_HD __forceinline__ void m3_vec(const double* A, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
PI_HD __forceinline__ void m3_tvec(const double* A, const double* x, double* y) {     // A^T x
#pragma unroll
  for (int i = 0; i < 3; i++) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}
PI_HD __forceinline__ void m3_skew(const double* w, double* W) {
  W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
// I + a W + b W^2
PI_HD __forceinline__ void m3_rodrigues(const double* w, double a, double b, double* R) {
  double W[9], W2[9];
  m3_skew(w, W);
  m3_mul(W, W, W2);
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = ((i & 3) == 0 ? 1.0 : 0.0) + a * W[i] + b * W2[i];
}
// the four SO3 functions of S/G2oTypes.cc:986-1063 with their small-angle branches at 1e-5; ExpSO3 without the float round trip and the
// SVD behind it (the closed form is orthonormal to rounding)
PI_HD inline void pi_exp_so3(const double* w, double* R) {
  const double d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = sqrt(d2);
  if (d < 1e-5) m3_rodrigues(w, 1.0, 0.5, R);
  else m3_rodrigues(w, sin(d) / d, (1.0 - cos(d)) / d2, R);
}
PI_HD inline void pi_log_so3(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
  const double costheta = (tr - 1.0) * 0.5;
  if (costheta > 1 || costheta < -1) return;
  const double theta = acos(costheta), s = sin(theta);
  if (fabs(s) < 1e-5) return;
#pragma unroll
  for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}
PI_HD inline void pi_right_jacobian(const double* v, double* J) {
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
  if (d < 1e-5) m3_rodrigues(v, 0.0, 0.0, J);
  else m3_rodrigues(v, -(1.0 - cos(d)) / d2, (d - sin(d)) / (d2 * d), J);
}
PI_HD inline void pi_inv_right_jacobian(const double* v, double* J) {
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
  if (d < 1e-5) m3_rodrigues(v, 0.0, 0.0, J);
  else m3_rodrigues(v, 0.5, 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d)), J);
}
// IMU::NormalizeRotation (S/ImuTypes.cc:30-36), U V^T of the SVD = the orthogonal polar factor: Newton's iteration X <- (X + X^-T) / 2,
// quadratic from the 1e-7 a float dR is away from a rotation (three steps reach rounding)
PI_HD inline void pi_normalize_rotation(double* X) {
#pragma unroll 1
  for (int it = 0; it < 3; it++) {
    double C[9];                                      // cofactors: X^-T = C / det
    C[0] = X[4] * X[8] - X[5] * X[7]; C[1] = X[5] * X[6] - X[3] * X[8]; C[2] = X[3] * X[7] - X[4] * X[6];
    C[3] = X[2] * X[7] - X[1] * X[8]; C[4] = X[0] * X[8] - X[2] * X[6]; C[5] = X[1] * X[6] - X[0] * X[7];
    C[6] = X[1] * X[5] - X[2] * X[4]; C[7] = X[2] * X[3] - X[0] * X[5]; C[8] = X[0] * X[4] - X[1] * X[3];
    const double det = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
#pragma unroll
    for (int i = 0; i < 9; i++) X[i] = 0.5 * (X[i] + C[i] / det);
  }
}
// rho0 / rho1 of RobustKernelHuber::robustify from delta alone (lm_step.hpp, which the including unit has in front of this file)
PI_HD __forceinline__ void pi_huber(double e, double delta, double* rho0, double* rho1) { orbg_lm::lm_huber(e, delta, delta * delta, rho0, rho1); }

// ImuCamPose::Update (S/G2oTypes.cc:192-220; the renormalisation at :206 discards its result) + the oplus of the three plain vertices
PI_HD inline void pi_oplus(PiState* s, const double* dx) {
  double dt[3], E[9], Rn[9];
  m3_vec(s->R, dx + 3, dt);
  pi_exp_so3(dx, E);
  m3_mul(s->R, E, Rn);
#pragma unroll
  for (int i = 0; i < 3; i++) { s->t[i] += dt[i]; s->v[i] += dx[6 + i]; s->bg[i] += dx[9 + i]; s->ba[i] += dx[12 + i]; }
#pragma unroll
  for (int i = 0; i < 9; i++) s->R[i] = Rn[i];
}
// Rcw = Rcb Rwb^T, tcw = Rcb (-Rwb^T twb) + tcb -> cam[0..9), cam[9..12)
PI_HD inline void pi_camera_pose(const PiState& s, const double* Rcb, const double* tcb, double* cam) {
  double tbw[3], r[3];
  m3_mult(Rcb, s.R, cam);
  m3_tvec(s.R, s.t, tbw);
#pragma unroll
  for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
  m3_vec(Rcb, tbw, r);
#pragma unroll
  for (int i = 0; i < 3; i++) cam[9 + i] = r[i] + tcb[i];
}

// EdgeInertial::computeError + linearizeOplus (S/G2oTypes.cc:720-800) between s1 (the other end) and s2 (the frame) -> rows 0..8 of J
// (columns: s1's 15 from 0 where `with_prev`, s2's pose and velocity from `co`), the error in column `ce`
PI_HD inline void pi_inertial_edge(const PiParams& P, const PiState& s1, const PiState& s2, bool with_prev, int co, int ce, double* J) {
  const double dt = P.dT, g[3] = {0.0, 0.0, -(double)9.81f};                        // IMU::GRAVITY_VALUE is a float
  double dbg[3], dba[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { dbg[i] = s1.bg[i] - P.lbg[i]; dba[i] = s1.ba[i] - P.lba[i]; }
  // the bias-dependent deltas (S/ImuTypes.cc:404-431)
  double w[3], E[9], dR[9], a[3], c[3], dV[3], dP[3];
  m3_vec(P.JRg, dbg, w);
  pi_exp_so3(w, E);
  m3_mul(P.dR, E, dR);
  pi_normalize_rotation(dR);
  m3_vec(P.JVg, dbg, a); m3_vec(P.JVa, dba, c);
#pragma unroll
  for (int i = 0; i < 3; i++) dV[i] = P.dV[i] + a[i] + c[i];
  m3_vec(P.JPg, dbg, a); m3_vec(P.JPa, dba, c);
#pragma unroll
  for (int i = 0; i < 3; i++) dP[i] = P.dP[i] + a[i] + c[i];
  double R12[9], eR[9], er[3], invJr[9];
  m3_tmul(s1.R, s2.R, R12);                       // Rbw1 Rwb2
  m3_tmul(dR, R12, eR);
  pi_log_so3(eR, er);
  pi_inv_right_jacobian(er, invJr);
  double dv[3], dp[3], rv[3], rp[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    dv[i] = s2.v[i] - s1.v[i] - g[i] * dt;
    dp[i] = s2.t[i] - s1.t[i] - s1.v[i] * dt - g[i] * dt * dt / 2;
  }
  m3_tvec(s1.R, dv, rv);
  m3_tvec(s1.R, dp, rp);
#pragma unroll
  for (int i = 0; i < 3; i++) { J[i * kPiLd + ce] = er[i]; J[(3 + i) * kPiLd + ce] = rv[i] - dV[i]; J[(6 + i) * kPiLd + ce] = rp[i] - dP[i]; }
  // pose 2: rotation invJr, translation Rbw1 Rwb2; velocity 2: Rbw1
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      J[i * kPiLd + co + j] = invJr[3 * i + j];
      J[(6 + i) * kPiLd + co + 3 + j] = R12[3 * i + j];
      J[(3 + i) * kPiLd + co + 6 + j] = s1.R[3 * j + i];
    }
  if (!with_prev) return;
  double T[9], T2[9], S[9], Jr[9];
  m3_tmul(s2.R, s1.R, T);                         // Rwb2^T Rwb1
  m3_mul(invJr, T, T2);
  double Sv[9], Sp[9];
  m3_skew(rv, Sv); m3_skew(rp, Sp);
  pi_right_jacobian(w, Jr);
  m3_mult(invJr, eR, T);                          // invJr eR^T
  m3_mul(T, Jr, S);
  m3_mul(S, P.JRg, T);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int k = 3 * i + j;
      J[i * kPiLd + j] = -T2[k];                                  // pose 1, rotation
      J[(3 + i) * kPiLd + j] = Sv[k];
      J[(6 + i) * kPiLd + j] = Sp[k];
      J[(6 + i) * kPiLd + 3 + j] = i == j ? -1.0 : 0.0;           // pose 1, translation
      J[(3 + i) * kPiLd + 6 + j] = -s1.R[3 * j + i];              // velocity 1
      J[(6 + i) * kPiLd + 6 + j] = -s1.R[3 * j + i] * dt;
      J[i * kPiLd + 9 + j] = -T[k];                               // gyro bias 1
      J[(3 + i) * kPiLd + 9 + j] = -P.JVg[k];
      J[(6 + i) * kPiLd + 9 + j] = -P.JPg[k];
      J[(3 + i) * kPiLd + 12 + j] = -P.JVa[k];                    // accelerometer bias 1
      J[(6 + i) * kPiLd + 12 + j] = -P.JPa[k];
    }
}
// EdgeGyroRW, EdgeAccRW (I/G2oTypes.h:632-701): rows 9..14; EdgePriorPoseImu (S/G2oTypes.cc:929-969): rows 15..29
PI_HD inline void pi_walk_prior_edges(const PiParams& P, const PiState& s1, const PiState& s2, bool with_prev, int co, int ce, double* J) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    J[(9 + i) * kPiLd + ce] = s2.bg[i] - s1.bg[i];
    J[(12 + i) * kPiLd + ce] = s2.ba[i] - s1.ba[i];
    J[(9 + i) * kPiLd + co + 9 + i] = 1.0;
    J[(12 + i) * kPiLd + co + 12 + i] = 1.0;
    if (with_prev) { J[(9 + i) * kPiLd + 9 + i] = -1.0; J[(12 + i) * kPiLd + 12 + i] = -1.0; }
  }
  if (!with_prev) return;
  double Rr[9], er[3], dtv[3], et[3], iJ[9];
  m3_tmul(P.prior.R, s1.R, Rr);
  pi_log_so3(Rr, er);
  pi_inv_right_jacobian(er, iJ);
#pragma unroll
  for (int i = 0; i < 3; i++) dtv[i] = s1.t[i] - P.prior.t[i];
  m3_tvec(P.prior.R, dtv, et);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    J[(15 + i) * kPiLd + ce] = er[i];
    J[(18 + i) * kPiLd + ce] = et[i];
    J[(21 + i) * kPiLd + ce] = s1.v[i] - P.prior.v[i];
    J[(24 + i) * kPiLd + ce] = s1.bg[i] - P.prior.bg[i];
    J[(27 + i) * kPiLd + ce] = s1.ba[i] - P.prior.ba[i];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      J[(15 + i) * kPiLd + j] = iJ[3 * i + j];
      J[(18 + i) * kPiLd + 3 + j] = Rr[3 * i + j];
    }
    J[(21 + i) * kPiLd + 6 + i] = 1.0; J[(24 + i) * kPiLd + 9 + i] = 1.0; J[(27 + i) * kPiLd + 12 + i] = 1.0;
  }
}

// one visual edge at the camera pose `cam`: error (third 0 for a monocular edge), chi2, camera-frame point
struct PiVis { double e[3], c2, Xc[3]; };
PI_HD __forceinline__ void pi_visual_error(const double* cam, const PiParams& P, const float* X, float u, float v, float ur, double om, PiVis* o) {
  const double x = X[0], y = X[1], z = X[2];
#pragma unroll
  for (int i = 0; i < 3; i++) o->Xc[i] = cam[3 * i] * x + cam[3 * i + 1] * y + cam[3 * i + 2] * z + cam[9 + i];
  // ImuCamPose::Project / ProjectStereo (S/G2oTypes.cc:170-185) through Pinhole::project
  const double pu = P.fx * o->Xc[0] / o->Xc[2] + P.cx, pv = P.fy * o->Xc[1] / o->Xc[2] + P.cy;
  o->e[0] = (double)u - pu;
  o->e[1] = (double)v - pv;
  o->e[2] = ur < 0 ? 0.0 : (double)ur - (pu - P.bf * (1.0 / o->Xc[2]));
  o->c2 = o->e[0] * (om * o->e[0]) + o->e[1] * (om * o->e[1]) + o->e[2] * (om * o->e[2]);
}
// J^T (w Omega) J (21, upper triangle row-major) and -J^T (w Omega) e (6) of one visual edge, added to acc[0..27)
// (EdgeMonoOnlyPose / EdgeStereoOnlyPose::linearizeOplus, S/G2oTypes.cc:375-395, 484-508: proj_jac Rcb SE3deriv(Xb), Xb = Rbc Xc + tbc)
PI_HD __forceinline__ void pi_visual_hessian(const PiVis& o, const PiParams& P, const double* tbc, bool mono, double w, double* acc) {
  const double x = o.Xc[0], y = o.Xc[1], z = o.Xc[2], iz2 = 1.0 / (z * z);
  double pj[9] = {P.fx / z, 0.0, -P.fx * x * iz2, 0.0, P.fy / z, -P.fy * y * iz2, 0.0, 0.0, 0.0};
  if (!mono) { pj[6] = pj[0]; pj[8] = pj[2] + P.bf * iz2; }
  double M[9], Xb[3];
  m3_mul(pj, P.Rcb, M);
  m3_tvec(P.Rcb, o.Xc, Xb);
#pragma unroll
  for (int i = 0; i < 3; i++) Xb[i] += tbc[i];
  double Jm[18];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    Jm[6 * k] = -M[3 * k + 1] * Xb[2] + M[3 * k + 2] * Xb[1];
    Jm[6 * k + 1] = M[3 * k] * Xb[2] - M[3 * k + 2] * Xb[0];
    Jm[6 * k + 2] = -M[3 * k] * Xb[1] + M[3 * k + 1] * Xb[0];
    Jm[6 * k + 3] = M[3 * k]; Jm[6 * k + 4] = M[3 * k + 1]; Jm[6 * k + 5] = M[3 * k + 2];
  }
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int c = a; c < 6; c++) acc[q++] += Jm[a] * (w * Jm[c]) + Jm[6 + a] * (w * Jm[6 + c]) + Jm[12 + a] * (w * Jm[12 + c]);
#pragma unroll
  for (int a = 0; a < 6; a++) acc[q++] -= Jm[a] * (w * o.e[0]) + Jm[6 + a] * (w * o.e[1]) + Jm[12 + a] * (w * o.e[2]);
}

// ---- Optimizer::InertialOptimization (inertial_init.hip): EdgeInertialGS (S/G2oTypes.cc:802-927) between two FIXED poses.  What one edge
// reads of its IMU::Preintegrated, widened to double by the host, and its information (orbg_imu_information: the constructor at
// :809-821 conditions it exactly as EdgeInertial's at :702-714 does).
struct PiGsEdge {
  int k1, k2;                          // mPrevKF, the keyframe
  double dT, dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], lbg[3], lba[3];
  double info9[81];
};
constexpr int kGsLd = 16;              // row stride of an edge's 9 x 16 block: [v1 3 | v2 3 | bg 3 | ba 3 | gdir 2 | s 1 | e 1]
enum { kGsColV1 = 0, kGsColV2 = 3, kGsColBg = 6, kGsColBa = 9, kGsColGd = 12, kGsColS = 14, kGsColE = 15 };
enum { kGsVel = 1, kGsBias = 2, kGsGdir = 4, kGsScale = 8, kGsAll = 15 };   // the column groups whose vertices are free

// EdgeInertialGS::computeError (:826-849) -> column kGsColE of J, and linearizeOplus (:851-927) for the column groups in `groups` (a fixed
// vertex is not a variable: its columns are neither computed nor written).  R1, t1, v1: mPrevKF's; R2, t2, v2: the keyframe's; bg, ba: the
// one bias every edge shares; Rwg, s: VertexGDir's and VertexScale's estimates.  The pose columns do not exist: every pose is fixed.
PI_HD inline void pi_inertial_gs_edge(const PiGsEdge& E, const double* R1, const double* t1, const double* v1, const double* R2, const double* t2,
                                      const double* v2, const double* bg, const double* ba, const double* Rwg, double s, int groups, double* J) {
  const double dt = E.dT, G = (double)9.81f;                                          // IMU::GRAVITY_VALUE is a float
  double dbg[3], dba[3], g[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { dbg[i] = bg[i] - E.lbg[i]; dba[i] = ba[i] - E.lba[i]; g[i] = Rwg[3 * i + 2] * -G; }   // Rwg gI, gI = (0, 0, -G)
  double w[3], X[9], dR[9], a[3], c[3], dV[3], dP[3];
  m3_vec(E.JRg, dbg, w);
  pi_exp_so3(w, X);
  m3_mul(E.dR, X, dR);
  pi_normalize_rotation(dR);
  m3_vec(E.JVg, dbg, a); m3_vec(E.JVa, dba, c);
#pragma unroll
  for (int i = 0; i < 3; i++) dV[i] = E.dV[i] + a[i] + c[i];
  m3_vec(E.JPg, dbg, a); m3_vec(E.JPa, dba, c);
#pragma unroll
  for (int i = 0; i < 3; i++) dP[i] = E.dP[i] + a[i] + c[i];
  double R12[9], eR[9], er[3];
  m3_tmul(R1, R2, R12);
  m3_tmul(dR, R12, eR);
  pi_log_so3(eR, er);
  double dvv[3], dpp[3], dv[3], dp[3], rv[3], rp[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    dvv[i] = v2[i] - v1[i];
    dpp[i] = t2[i] - t1[i] - v1[i] * dt;
    dv[i] = s * dvv[i] - g[i] * dt;
    dp[i] = s * dpp[i] - g[i] * dt * dt / 2;
  }
  m3_tvec(R1, dv, rv);
  m3_tvec(R1, dp, rp);
#pragma unroll
  for (int i = 0; i < 3; i++) { J[i * kGsLd + kGsColE] = er[i]; J[(3 + i) * kGsLd + kGsColE] = rv[i] - dV[i]; J[(6 + i) * kGsLd + kGsColE] = rp[i] - dP[i]; }
  if (groups & kGsVel) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double rb = R1[3 * j + i];                                              // Rbw1
        J[i * kGsLd + kGsColV1 + j] = 0.0; J[(3 + i) * kGsLd + kGsColV1 + j] = -s * rb; J[(6 + i) * kGsLd + kGsColV1 + j] = -s * rb * dt;
        J[i * kGsLd + kGsColV2 + j] = 0.0; J[(3 + i) * kGsLd + kGsColV2 + j] = s * rb; J[(6 + i) * kGsLd + kGsColV2 + j] = 0.0;
      }
  }
  if (groups & kGsBias) {
    double invJr[9], Jr[9], T[9], S[9];
    pi_inv_right_jacobian(er, invJr);
    pi_right_jacobian(w, Jr);
    m3_mult(invJr, eR, T);                                                            // invJr eR^T
    m3_mul(T, Jr, S);
    m3_mul(S, E.JRg, T);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int k = 3 * i + j;
        J[i * kGsLd + kGsColBg + j] = -T[k]; J[(3 + i) * kGsLd + kGsColBg + j] = -E.JVg[k]; J[(6 + i) * kGsLd + kGsColBg + j] = -E.JPg[k];
        J[i * kGsLd + kGsColBa + j] = 0.0; J[(3 + i) * kGsLd + kGsColBa + j] = -E.JVa[k]; J[(6 + i) * kGsLd + kGsColBa + j] = -E.JPa[k];
      }
  }
  if (groups & kGsGdir) {
    // dGdTheta = Rwg Gm, Gm(0, 1) = -G, Gm(1, 0) = G
    double d0[3], d1[3], r0[3], r1[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { d0[i] = Rwg[3 * i + 1] * G; d1[i] = Rwg[3 * i] * -G; }
    m3_tvec(R1, d0, r0);
    m3_tvec(R1, d1, r1);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      J[i * kGsLd + kGsColGd] = 0.0; J[i * kGsLd + kGsColGd + 1] = 0.0;
      J[(3 + i) * kGsLd + kGsColGd] = -r0[i] * dt; J[(3 + i) * kGsLd + kGsColGd + 1] = -r1[i] * dt;
      J[(6 + i) * kGsLd + kGsColGd] = -0.5 * r0[i] * dt * dt; J[(6 + i) * kGsLd + kGsColGd + 1] = -0.5 * r1[i] * dt * dt;
    }
  }
  if (groups & kGsScale) {
    double r0[3], r1[3];
    m3_tvec(R1, dvv, r0);
    m3_tvec(R1, dpp, r1);
#pragma unroll
    for (int i = 0; i < 3; i++) { J[i * kGsLd + kGsColS] = 0.0; J[(3 + i) * kGsLd + kGsColS] = r0[i]; J[(6 + i) * kGsLd + kGsColS] = r1[i]; }
  }
}
// GDirection::Update (I/G2oTypes.h:261-264): Rwg ExpSO3(u0, u1, 0); VertexScale::oplusImpl (:311-313): s exp(u)
PI_HD inline void pi_gdir_oplus(double* Rwg, double u0, double u1) {
  const double u[3] = {u0, u1, 0.0};
  double X[9], Rn[9];
  pi_exp_so3(u, X);
  m3_mul(Rwg, X, Rn);
#pragma unroll
  for (int i = 0; i < 9; i++) Rwg[i] = Rn[i];
}
