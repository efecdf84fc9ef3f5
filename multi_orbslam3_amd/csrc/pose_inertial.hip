// liborbgpu -- Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame for gfx950 (MI355X): the whole solve in one kernel launch
// (include/orbgpu.h: pose_inertial_optimize).
#include <time.h>

#include <cmath>

#include "common.hpp"
#include "wave.hpp"
#include "lm_block.hpp"
#include "sym_jacobi.hpp"

using namespace orbg;

// ------------------------------------------------------------------------------------------------
// S/Optimizer.cc:7603-7996 (LastKeyFrame: the frame's pose, velocity and biases, 15 unknowns) and :7998-8424 (LastFrame: the previous
// frame's 15 in front, 30 unknowns).  Gauss-Newton (G/core/optimization_algorithm_gauss_newton.cpp:50-93), dense solve, no accept /
// reject: 4 rounds of exactly 10 iterations unless a factorisation fails.
//
// One 256-thread workgroup; thread t owns correspondences t, t + 256, ...  Per iteration:
//   1. thread 0 linearises EdgeInertial (S/G2oTypes.cc:720-800), thread 64 the two random-walk edges and EdgePriorPoseImu (:929-969),
//      into the stacked Jacobian s_J (rows: inertial 9, gyro walk 3, accelerometer walk 3, prior 15; one more column holds the error),
//      while every thread linearises its visual edges (:375-395, 484-508) into 21 + 6 + 1 sums;
//   2. the visual sums are reduced in a fixed order (lm_block_reduce);
//   3. W J and W e, W the block-diagonal of the edges' information matrices: one entry per thread and pass;
//   4. H = J^T (w W J), b = -J^T (w W e), w the Huber weight of a row's edge (only the prior has a kernel), plus the visual 6 x 6;
//   5. wavefront 0 solves H x = b by LDL^T, lane i holding row i (lane_ldlt_solve, lambda = 0);
//   6. thread 0 updates the frame's vertices and the camera pose, thread 64 the previous frame's.
// All of it in double.  Every sum has a fixed order: the result is bit-reproducible from run to run.
namespace {

constexpr int kPiThreads = 256;
constexpr int kPiMaxN = 4096;
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
// what the kernel leaves in the staging block next to the outlier flags; stats: nBad, rounds run, solve failed, .., [7] = the
// sequence number that completes the record
struct PiOut { PiState cur; double chi2[4]; double H[900]; int stats[8]; };

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
// rho0 / rho1 of RobustKernelHuber::robustify (G/core/robust_kernel_impl.cpp:78-91)
PI_HD __forceinline__ void pi_huber(double e, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.0; }
  else { const double sq = sqrt(e); *rho0 = 2 * sq * delta - dsqr; *rho1 = delta / sq; }
}

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

// first row and width of the information block that row r of the stacked Jacobian belongs to
PI_HD __forceinline__ void pi_row_block(int r, int* r0, int* bw) {
  if (r < 9) { *r0 = 0; *bw = 9; }
  else if (r < 12) { *r0 = 9; *bw = 3; }
  else if (r < 15) { *r0 = 12; *bw = 3; }
  else { *r0 = 15; *bw = 15; }
}

template <int NU>      // 15: LastKeyFrame, 30: LastFrame
__global__ __launch_bounds__(kPiThreads) void pose_inertial_kernel(const PiParams* __restrict__ gP, const float* __restrict__ Xw, const float* __restrict__ ou,
                                                                  const float* __restrict__ ov, const float* __restrict__ our, const float* __restrict__ oinv,
                                                                  const uint8_t* __restrict__ oclose, PiOut* __restrict__ out,
                                                                  uint8_t* __restrict__ outlier_out, unsigned seq) {
  constexpr bool kPrev = NU == 30;
  constexpr int co = NU - 15;        // first column of the frame's unknowns
  constexpr int NR = NU;             // rows of the stacked Jacobian: 15 without the prior edge, 30 with it
  constexpr int ce = NU;             // the error column
  __shared__ PiParams P;
  __shared__ double s_J[30 * kPiLd], s_WJ[30 * kPiLd], s_H[30 * kPiLd], s_W[30 * 15];
  __shared__ double s_x[32];
  __shared__ int s_ok;
  __shared__ PiState s_cur, s_oth;
  __shared__ double s_cam[12], s_tbc[3];
  __shared__ double s_acc[28 * kLmRow], s_part[28 * 8], red[28];
  __shared__ double s_wsum[2][4];
  __shared__ double s_chi2[kPiMaxN];                     // the error every visual edge holds (chi2 of its last computeError)
  __shared__ uint8_t s_out[kPiMaxN];                     // mvbOutlier
  const int tid = threadIdx.x;
  int sum_slot = 0;
  {
    const double* src = reinterpret_cast<const double*>(gP);
    double* dst = reinterpret_cast<double*>(&P);
    for (int i = tid; i < (int)(sizeof(PiParams) / sizeof(double)); i += kPiThreads) dst[i] = src[i];
  }
  for (int i = tid; i < 30 * kPiLd; i += kPiThreads) { s_J[i] = 0; s_WJ[i] = 0; s_H[i] = 0; }
  __syncthreads();
  const int n = P.n;
  for (int i = tid; i < n; i += kPiThreads) { s_chi2[i] = 0; s_out[i] = 0; }
  // the block-diagonal information: row r holds its block's row
  for (int i = tid; i < NR * 15; i += kPiThreads) {
    const int r = i / 15, k = i % 15;
    int r0, bw;
    pi_row_block(r, &r0, &bw);
    double w = 0;
    if (k < bw) w = r < 9 ? P.info9[9 * r + k] : r < 12 ? P.infoG[3 * (r - 9) + k] : r < 15 ? P.infoA[3 * (r - 12) + k] : P.priorH[15 * (r - 15) + k];
    s_W[i] = w;
  }
  if (tid == 0) {
    s_cur = P.cur; s_oth = P.oth;
    pi_camera_pose(s_cur, P.Rcb, P.tcb, s_cam);
    double t[3];
    m3_tvec(P.Rcb, P.tcb, t);                            // tbc = -Rbc tcb
    for (int i = 0; i < 3; i++) s_tbc[i] = -t[i];
    for (int i = 0; i < 4; i++) out->chi2[i] = 0;
  }
  __syncthreads();
  const double dM = (float)sqrt(5.991), dS = (float)sqrt(7.815);
  const double tbc[3] = {s_tbc[0], s_tbc[1], s_tbc[2]};
  const bool last_frame = kPrev;
  bool robust = true, failed = false;
  int nBad = 0, nInl = 0, rounds = 0;

  // steps 1-4 of an iteration at the current estimates; weights: the Huber weights of the solve, else the plain Hessian of the result.
  // Leaves H in s_H (columns 0..NU) and b in column NU; returns the robustified chi2 of the active edges (valid in thread 0).
  auto build = [&](bool weights) -> double {
    if (tid == 0) pi_inertial_edge(P, s_oth, s_cur, kPrev, co, ce, s_J);
    if (tid == 64) pi_walk_prior_edges(P, s_oth, s_cur, kPrev, co, ce, s_J);
    double cam[12];
#pragma unroll
    for (int i = 0; i < 12; i++) cam[i] = s_cam[i];
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; i++) acc[i] = 0;
    for (int i = tid; i < n; i += kPiThreads) {
      if (s_out[i]) continue;
      const float ur = our[i];
      const bool mono = ur < 0;
      const double om = (double)oinv[i];
      PiVis o;
      pi_visual_error(cam, P, Xw + 3 * (size_t)i, ou[i], ov[i], ur, om, &o);
      double rho0 = o.c2, rho1 = 1.0;
      if (weights) {
        s_chi2[i] = o.c2;                                // the error the edge holds from now on
        if (robust) pi_huber(o.c2, mono ? dM : dS, &rho0, &rho1);
        acc[27] += rho0;
      }
      pi_visual_hessian(o, P, tbc, mono, rho1 * om, acc);
    }
    lm_block_reduce<28>(acc, s_acc, s_part, red);          // (its barriers also publish s_J)
    // W J and W e
    for (int id = tid; id < NR * (NU + 1); id += kPiThreads) {
      const int r = id / (NU + 1), c = id % (NU + 1);
      int r0, bw;
      pi_row_block(r, &r0, &bw);
      double s = 0;
      for (int k = 0; k < bw; k++) s += s_W[r * 15 + k] * s_J[(r0 + k) * kPiLd + c];
      s_WJ[r * kPiLd + c] = s;
    }
    __syncthreads();
    // the prior edge's Huber kernel (delta 5, never removed)
    double wp = 1.0, rho0p = 0.0;
    if (kPrev) {
      double c2 = 0;
      for (int r = 15; r < 30; r++) c2 += s_J[r * kPiLd + ce] * s_WJ[r * kPiLd + ce];
      rho0p = c2;
      if (weights) pi_huber(c2, 5.0, &rho0p, &wp);
    }
    for (int id = tid; id < NU * (NU + 1); id += kPiThreads) {
      const int a = id / (NU + 1), c = id % (NU + 1);
      double s = 0;
      for (int r = 0; r < 15; r++) s += s_J[r * kPiLd + a] * s_WJ[r * kPiLd + c];
      if (kPrev) {
        double sp = 0;
        for (int r = 15; r < 30; r++) sp += s_J[r * kPiLd + a] * s_WJ[r * kPiLd + c];
        s += wp * sp;
      }
      if (c == ce) s = -s;
      if (a >= co && a < co + 6) {
        const int av = a - co;
        if (c == ce) s += red[21 + av];
        else if (c >= co && c < co + 6) {
          const int cv = c - co, lo = min(av, cv), hi = max(av, cv);
          s += red[lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];
        }
      }
      s_H[a * kPiLd + c] = s;
    }
    double chi = 0;
    if (tid == 0) {
      for (int r = 0; r < 15; r++) chi += s_J[r * kPiLd + ce] * s_WJ[r * kPiLd + ce];
      chi += red[27] + rho0p;
    }
    __syncthreads();
    return chi;
  };

  for (int round = 0; round < 4; round++) {
    rounds = round + 1;
    for (int it = 0; it < 10; it++) {
      const double chi = build(true);
      if (tid == 0) out->chi2[round] = chi;
      if (tid < 64) {
        const int li = min(tid, NU - 1);
        double Hrow[NU];
#pragma unroll
        for (int j = 0; j < NU; j++) Hrow[j] = s_H[li * kPiLd + j];
        double x[NU];
#pragma unroll
        for (int j = 0; j < NU; j++) x[j] = 0;
        const bool ok = lane_ldlt_solve<NU, true>(Hrow, s_H[li * kPiLd + ce], li, 0.0, x);
        if (tid == 0) {
#pragma unroll
          for (int j = 0; j < NU; j++) s_x[j] = x[j];
          s_ok = ok ? 1 : 0;
        }
      }
      __syncthreads();
      if (!s_ok) { failed = true; break; }                // (uniform: every thread reads the same word; nothing is applied)
      if (tid == 0) { pi_oplus(&s_cur, s_x + co); pi_camera_pose(s_cur, P.Rcb, P.tcb, s_cam); }
      if (kPrev && tid == 64) pi_oplus(&s_oth, s_x);
      __syncthreads();
    }
    // ---- classification (S/Optimizer.cc:7836-7916, 8246-8324): an excluded edge gets a fresh error at the final estimate, an active one
    // keeps the error of the round's last linearisation; the comparison is in float; isDepthPositive() at the final estimate
    const float thM = last_frame ? 5.991f : (round == 0 ? 12.f : round == 1 ? 7.5f : 5.991f);
    const float thC = (float)(1.5 * (double)thM);
    const float thS = round == 0 ? 15.6f : round == 1 ? 9.8f : 7.815f;
    double bl = 0;
    {
      double cam[12];
#pragma unroll
      for (int i = 0; i < 12; i++) cam[i] = s_cam[i];
      for (int i = tid; i < n; i += kPiThreads) {
        const float ur = our[i];
        const bool mono = ur < 0;
        PiVis o;
        pi_visual_error(cam, P, Xw + 3 * (size_t)i, ou[i], ov[i], ur, (double)oinv[i], &o);
        if (s_out[i]) s_chi2[i] = o.c2;
        const float c2f = (float)s_chi2[i];
        bool bad;
        if (mono) bad = (c2f > (oclose[i] ? thC : thM)) || !(o.Xc[2] > 0.0);
        else bad = c2f > thS;
        s_out[i] = bad;
        bl += bad;
      }
    }
    nBad = (int)block_sum(bl, s_wsum, sum_slot); sum_slot ^= 1;
    nInl = n - nBad;
    if (round == 2) robust = false;                        // setRobustKernel(0) on the visual edges
    if (n + (kPrev ? 4 : 3) < 10) break;                   // optimizer.edges().size() < 10
  }
  // ---- recovery (S/Optimizer.cc:7919-7946, 8327-8355): every visual edge gets a fresh error; compared in double
  if (nInl < 30 && !P.rec_init) {
    double cam[12];
#pragma unroll
    for (int i = 0; i < 12; i++) cam[i] = s_cam[i];
    double bl = 0;
    for (int i = tid; i < n; i += kPiThreads) {
      const float ur = our[i];
      PiVis o;
      pi_visual_error(cam, P, Xw + 3 * (size_t)i, ou[i], ov[i], ur, (double)oinv[i], &o);
      if (o.c2 < (ur < 0 ? 18.0 : 24.0)) s_out[i] = 0;
      else bl += 1.0;
    }
    nBad = (int)block_sum(bl, s_wsum, sum_slot); sum_slot ^= 1;
  }
  __syncthreads();
  // ---- the Hessian for the next frame's prior: the final estimate, no robust weights, the correspondences that are not outliers
  build(false);
  for (int id = tid; id < NU * NU; id += kPiThreads) out->H[id] = s_H[(id / NU) * kPiLd + id % NU];
  for (int i = tid; i < n; i += kPiThreads) outlier_out[i] = s_out[i];
  if (tid == 0) {
    out->cur = s_cur;
    out->stats[0] = nBad; out->stats[1] = rounds; out->stats[2] = failed ? 1 : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");              // system-scope release of every wavefront's results (no acquire half)
  __syncthreads();
  if (tid == 0) *reinterpret_cast<volatile int*>(&out->stats[7]) = (int)seq;   // results are complete: the host spins on this word
}

// the calling thread's work area (common.hpp; the reference calls a static member: no handle)
struct PiBufs {
  orbg::StageBlock stage;
  void release_buffers() { stage.release(); }
};
WorkArea<PiBufs>& pi_work() { static thread_local WorkArea<PiBufs> w; return w; }

void pi_widen_state(const pose_inertial_state& s, PiState* d) {
  for (int i = 0; i < 9; i++) d->R[i] = s.Rwb[i];
  for (int i = 0; i < 3; i++) { d->t[i] = s.twb[i]; d->v[i] = s.vwb[i]; d->bg[i] = s.bg[i]; d->ba[i] = s.ba[i]; }
}

// the problem as the kernel reads it: every float widened to double
void pi_fill_params(const pose_inertial_problem& prob, PiParams* P) {
  const pose_inertial_problem* p = &prob;
  memset(P, 0, sizeof(PiParams));
  P->n = p->n; P->form = p->form; P->rec_init = p->rec_init;
  P->fx = p->fx; P->fy = p->fy; P->cx = p->cx; P->cy = p->cy; P->bf = p->bf;
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) P->Rcb[3 * i + j] = p->Tcb[4 * i + j]; P->tcb[i] = p->Tcb[4 * i + 3]; }
  pi_widen_state(p->frame, &P->cur);
  pi_widen_state(p->other, &P->oth);
  const pose_inertial_preint& I = p->preint;
  P->dT = I.dT;
  for (int i = 0; i < 9; i++) { P->dR[i] = I.dR[i]; P->JRg[i] = I.JRg[i]; P->JVg[i] = I.JVg[i]; P->JVa[i] = I.JVa[i]; P->JPg[i] = I.JPg[i]; P->JPa[i] = I.JPa[i]; }
  for (int i = 0; i < 3; i++) { P->dV[i] = I.dV[i]; P->dP[i] = I.dP[i]; P->lbg[i] = I.bg[i]; P->lba[i] = I.ba[i]; }
  memcpy(P->info9, p->info9, sizeof(P->info9)); memcpy(P->infoG, p->infoG, sizeof(P->infoG)); memcpy(P->infoA, p->infoA, sizeof(P->infoA));
  if (p->form == POSE_INERTIAL_LAST_FRAME) {
    const pose_inertial_prior& c = *p->prior;
    memcpy(P->prior.R, c.Rwb, sizeof(c.Rwb)); memcpy(P->prior.t, c.twb, sizeof(c.twb)); memcpy(P->prior.v, c.vwb, sizeof(c.vwb));
    memcpy(P->prior.bg, c.bg, sizeof(c.bg)); memcpy(P->prior.ba, c.ba, sizeof(c.ba)); memcpy(P->priorH, c.H, sizeof(c.H));
  }
}

// Optimizer::Marginalize(H, 0, 14) (S/Optimizer.cc:5228-5308) of the 30 x 30, its lower-right 15 x 15: Hcc - Hcb pinv(Hbb) Hbc with the
// singular values of Hbb up to 1e-6 dropped.  Hbb is symmetric: its singular values are the magnitudes of its eigenvalues and V s^-1 U^T
// is sum(1 / lambda v v^T).
void pi_marginalize(const double* H30, double* H15) {
  double Hbb[225], w[15], V[225], inv[225];
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) Hbb[15 * i + j] = H30[30 * i + j];
  sym_eig_jacobi(15, Hbb, w, V);
  sym_rebuild(15, w, V, [](double l) { return std::fabs(l) > 1e-6 ? 1.0 / l : 0.0; }, inv);
  double T[225];                                  // pinv(Hbb) Hbc
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = 0;
      for (int k = 0; k < 15; k++) s += inv[15 * i + k] * H30[30 * k + 15 + j];
      T[15 * i + j] = s;
    }
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = 0;
      for (int k = 0; k < 15; k++) s += H30[30 * (15 + i) + k] * T[15 * k + j];
      H15[15 * i + j] = H30[30 * (15 + i) + 15 + j] - s;
    }
}

}  // namespace

// the calling thread's pose_inertial_optimize calls on `device` use the caller's stream from now on (NULL: the library's M stream again)
extern "C" int pose_inertial_set_stream(int device, void* hip_stream) {
  WorkArea<PiBufs>& sc = pi_work();
  int rc = sc.open(device, "po");
  if (rc) return rc;
  return orbg::swap_stream(&sc.stream, &sc.ext_stream, hip_stream, "po");
}

// cv::Mat::inv(cv::DECOMP_SVD) of a symmetric block of C in double (singular values below 2 eps of their sum dropped, as OpenCV's
// back-substitution does), read back as float
static void pi_block_information(const float* C, int r0, int m, double* info) {
  double A[81], w[9], V[81];
  for (int i = 0; i < m; i++)
    for (int j = 0; j < m; j++) A[m * i + j] = 0.5 * ((double)C[15 * (r0 + i) + r0 + j] + (double)C[15 * (r0 + j) + r0 + i]);
  sym_eig_jacobi(m, A, w, V);
  double sum = 0;
  for (int i = 0; i < m; i++) sum += std::fabs(w[i]);
  const double cut = sum * 2.0 * 2.220446049250313e-16;
  sym_rebuild(m, w, V, [cut](double l) { return std::fabs(l) > cut ? 1.0 / l : 0.0; }, info);
  for (int i = 0; i < m * m; i++) info[i] = (double)(float)info[i];
}

extern "C" int orbg_imu_information(const float* C, double* info9, double* infoG, double* infoA) {
  if (!C || !info9 || !infoG || !infoA) return ORBG_BAD_ARG;
  double I9[81], w[9], V[81];
  pi_block_information(C, 0, 9, I9);
  pi_block_information(C, 9, 3, infoG);
  pi_block_information(C, 12, 3, infoA);
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 9; j++) info9[9 * i + j] = (I9[9 * i + j] + I9[9 * j + i]) / 2;          // S/G2oTypes.cc:707
  sym_eig_jacobi(9, info9, w, V);
  sym_rebuild(9, w, V, [](double l) { return l < 1e-12 ? 0.0 : l; }, info9);
  return ORBG_OK;
}

extern "C" int orbg_condition_prior(double* H) {
  if (!H) return ORBG_BAD_ARG;
  double w[15], V[225];
  sym_eig_jacobi(15, H, w, V);
  sym_rebuild(15, w, V, [](double l) { return l < 1e-12 ? 0.0 : l; }, H);
  return ORBG_OK;
}

static int pi_check_problem(const pose_inertial_problem* p) {
  if (!p || p->struct_size < sizeof(pose_inertial_problem)) return ORBG_BAD_ARG;
  if (p->form != POSE_INERTIAL_LAST_KEYFRAME && p->form != POSE_INERTIAL_LAST_FRAME) return ORBG_BAD_ARG;
  if (p->n_left != -1) return ORBG_BAD_ARG;                                  // a two-camera Frame: not supported
  if (p->n < 0 || (p->n > 0 && (!p->Xw || !p->u || !p->v || !p->ur || !p->inv_sigma2 || !p->close))) return ORBG_BAD_ARG;
  if (p->form == POSE_INERTIAL_LAST_FRAME && !p->prior) return ORBG_BAD_ARG;
  if (p->n > kPiMaxN) return ORBG_CAP_EXCEEDED;
  return ORBG_OK;
}

extern "C" int pose_inertial_host_linearize(const pose_inertial_problem* p, double* J, double* vis) {
  int rc = pi_check_problem(p);
  if (rc) return rc;
  if (!J || (p->n > 0 && !vis)) return ORBG_BAD_ARG;
  static thread_local PiParams P;
  pi_fill_params(*p, &P);
  const bool prev = p->form == POSE_INERTIAL_LAST_FRAME;
  const int nu = prev ? 30 : 15, co = nu - 15;
  for (int i = 0; i < 30 * kPiLd; i++) J[i] = 0;
  pi_inertial_edge(P, P.oth, P.cur, prev, co, nu, J);
  pi_walk_prior_edges(P, P.oth, P.cur, prev, co, nu, J);
  double cam[12], t[3], tbc[3];
  pi_camera_pose(P.cur, P.Rcb, P.tcb, cam);
  m3_tvec(P.Rcb, P.tcb, t);
  for (int i = 0; i < 3; i++) tbc[i] = -t[i];
  for (int i = 0; i < p->n; i++) {
    PiVis o;
    const double om = (double)p->inv_sigma2[i];
    pi_visual_error(cam, P, p->Xw + 3 * (size_t)i, p->u[i], p->v[i], p->ur[i], om, &o);
    double* out = vis + 31 * (size_t)i;
    for (int k = 0; k < 3; k++) out[k] = o.e[k];
    out[3] = o.c2;
    for (int k = 0; k < 27; k++) out[4 + k] = 0;
    pi_visual_hessian(o, P, tbc, p->ur[i] < 0, om, out + 4);
  }
  return ORBG_OK;
}

extern "C" int pose_inertial_optimize(const pose_inertial_problem* p, pose_inertial_result* r) {
  if (!r || r->struct_size < sizeof(pose_inertial_result)) return ORBG_BAD_ARG;
  if (p && p->n > 0 && !r->outlier) return ORBG_BAD_ARG;
  const int crc = pi_check_problem(p);
  if (crc) return crc;
  WorkArea<PiBufs>& sc = pi_work();
  int rc = sc.open(p->device, "po");
  if (rc) return rc;
  const int n = p->n;
  // one staging block: the result record and the flags are written in place (mapped); the parameters and the per-correspondence arrays,
  // which every iteration re-reads, get the block's one copy to the device
  orbg::StageBlock& S = sc.stage;
  if ((rc = S.begin(orbg::StageLayout::bound(10, sizeof(PiParams) + sizeof(PiOut) + (size_t)n * 30)))) return rc;
  const auto s_out = S.room<PiOut>(1);
  const auto s_flag = S.room<uint8_t>(n);
  const auto s_prm = S.room<PiParams>(1, true);
  const float* dX = S.add(p->Xw, 3 * (size_t)n, true);
  const float* du = S.add(p->u, n, true); const float* dv = S.add(p->v, n, true); const float* dur = S.add(p->ur, n, true);
  const float* dom = S.add(p->inv_sigma2, n, true);
  const uint8_t* dcl = S.add(p->close, n, true);
  pi_fill_params(*p, S.host(s_prm));
  if ((rc = S.commit(sc.stream))) return rc;
  static thread_local unsigned pi_seq = 0;
  pi_seq = (pi_seq + 1) & 0x7FFFFFFFu;
  if (pi_seq == 0) pi_seq = 1;
  PiOut* ho = S.host(s_out);
  volatile const int* seq_word = &ho->stats[7];
  ho->stats[7] = 0;
  if (p->form == POSE_INERTIAL_LAST_FRAME)
    hipLaunchKernelGGL(pose_inertial_kernel<30>, dim3(1), dim3(kPiThreads), 0, sc.stream, (const PiParams*)S.device(s_prm), dX, du, dv, dur, dom, dcl,
                       S.mapped(s_out), S.mapped(s_flag), pi_seq);
  else
    hipLaunchKernelGGL(pose_inertial_kernel<15>, dim3(1), dim3(kPiThreads), 0, sc.stream, (const PiParams*)S.device(s_prm), dX, du, dv, dur, dom, dcl,
                       S.mapped(s_out), S.mapped(s_flag), pi_seq);
  ORBG_HIP(hipGetLastError());
  {
    bool got = false;
    if (orbg::poll_allowed()) {
      timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
      for (unsigned spins = 0; !got; spins++) {
        if (*seq_word == (int)pi_seq) { got = true; break; }
        if ((spins & 0xFFFF) == 0xFFFF) {
          timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
          if ((t1.tv_sec - t0.tv_sec) * 1000.0 + (t1.tv_nsec - t0.tv_nsec) * 1e-6 > 100.0) break;
        }
      }
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    if (!got) ORBG_HIP(hipStreamSynchronize(sc.stream));
  }
  memcpy(r->Rwb, ho->cur.R, sizeof(r->Rwb)); memcpy(r->twb, ho->cur.t, sizeof(r->twb)); memcpy(r->vwb, ho->cur.v, sizeof(r->vwb));
  memcpy(r->bg, ho->cur.bg, sizeof(r->bg)); memcpy(r->ba, ho->cur.ba, sizeof(r->ba));
  memcpy(r->chi2, ho->chi2, sizeof(r->chi2));
  S.get(s_flag, r->outlier);
  r->n_bad = ho->stats[0];
  r->n_inliers = n - r->n_bad;
  r->rounds_run = ho->stats[1];
  r->solve_failed = ho->stats[2];
  if (p->form == POSE_INERTIAL_LAST_FRAME) pi_marginalize(ho->H, r->H);
  else memcpy(r->H, ho->H, sizeof(r->H));
  return ORBG_OK;
}
