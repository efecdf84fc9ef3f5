// Optimizer::OptimizeSim3 (S/Optimizer.cc:4031-4310, the overload LoopClosing calls at S/LoopClosing.cc:555 and :782) for gfx950:
// the whole refinement of one Sim3 -- both rounds, every Levenberg-Marquardt iteration and every accept / reject trial -- in ONE
// kernel launch, and the refinements of a whole batch of candidates in one launch too (include/orbgpu.h: orbm_sim3_optimize[_batch]).
//
// Grid = problems; one 256-thread workgroup owns one problem, thread t owns the edge pairs t, t + 256, ... (no cap on n: a problem of
// up to kTile pairs is staged in LDS once, a larger one is read from global memory on every pass).  A pair is the two edges the
// reference adds per kept match: EdgeSim3ProjectXYZ (obs1 - project1(S12.map(P3D2c))) and EdgeInverseSim3ProjectXYZ
// (obs2 - project2(S12.inverse().map(P3D1c))), I/OptimizableTypes.h:175-215.
//   Linearisation  both linearizeOplus overrides are commented out in the reference (I/OptimizableTypes.h:192,213): the Jacobians are
//                  g2o's central differences, delta = 1e-9, through oplusImpl (G/core/base_binary_edge.hpp:176-197).  The 14 perturbed
//                  estimates Sim3(+-delta e_d) * S12 and their inverses do not depend on the edge: lanes 0..14 compute them (and the
//                  unperturbed pair) once per linearisation into LDS, then every pair evaluates 1 + 14 map + project per side and
//                  forms its 2 x 7 Jacobians as scalar * (e+ - e-).  With fix_scale oplusImpl zeroes update[6] itself
//                  (I/OptimizableTypes.h:162-163): both perturbed estimates of column 7 are Sim3(0) * S12, the column is exactly 0.
//   Reductions     28 upper-triangle entries of H, 7 of b, the robustified chi2: a DPP tree inside each wavefront, then the four wave
//                  totals in wave order.  Fixed order: two runs give the same bits, and so does a problem alone or inside a batch (a
//                  workgroup sees nothing but its own problem).
//   Solve, control (H + lambda I) x = b on lanes 0..6 of every wavefront (lm_block.hpp, lane_ldlt_solve<7>: PoseOptimization runs the <6> form);
//                  lambda init, computeScale, the 1 - (2 rho - 1)^3 update, _ni, ten trials and the _nBad >= 3 stop as in
//                  G/core/optimization_algorithm_levenberg.cpp:61-194.  The LM state is kept identically in every thread (all of
//                  them read the same block sums and run the same arithmetic): the control flow needs no broadcast.
//   Rounds         optimize(5) with Huber; pairs with chi2 > th2 on either side leave (:4241 reads chi2() WITHOUT computeError(): the
//                  errors are those of the LAST TRIAL evaluated, accepted or not -- pop() restores estimates, not errors; the last
//                  chi2 of every pair is therefore kept); Huber off; nCorrespondences - nBad < 10: return 0 with the INPUT estimate
//                  (:4271); optimize(nBad > 0 ? 10 : 5) with lambda re-initialised; errors recomputed, second pass, nIn (:4279-4301).
// Comparisons keep the reference's form so that NaN and +-inf take its branches: chi2 > th2, rho > 0 && isfinite(tempChi),
// while (rho < 0 && ...), rho == 0, e <= dsqr, and std::max / std::min as the ternaries they are.  Nothing special-cases z <= 0.
// No atomics, no cooperative launch: a workgroup never waits for another one.
//
// Arithmetic.  Everything is FP64, -ffp-contract=off.  Eigen is not part of the reference's source; what it does inside a call is a
// choice made here (tests/sim3_opt_model.py restates the same ones, and is itself compared with a long double evaluation):
//   E-1  Quaterniond(Matrix3d): trace > 0: w = sqrt(trace + 1) / 2, vector part from the antisymmetric part times 0.5 / sqrt; else from
//        the largest diagonal entry (se3.hpp quat_from_R).  NOT renormalised, as Sim3(Vector7d) does not.
//   E-2  Quaterniond * Vector3d: uv = 2 (q.vec x v); v + w uv + q.vec x uv, added in that order (se3.hpp quat_rotate).
//   E-3  Quaterniond * Quaterniond: w = a.w b.w - a.x b.x - a.y b.y - a.z b.z, x = a.w b.x + a.x b.w + a.y b.z - a.z b.y, ...: left to right.
//   E-4  3 x 3 products (Omega * Omega, W * upsilon): row times column, added in k order; sums of matrices left to right.
//   E-5  Eigen::LDLT in LinearSolverDense (G/solvers/linear_solver_dense.h:65-113): no pivoting, ascending k, the step refused unless
//        every pivot is positive and finite (isPositive()); a refused solve leaves x as it was, and update() runs with that x.
//   E-6  map: s * (r * xyz) + t; inverse: (r*, r* * ((-1. / s) * t), 1. / s) as written in G/types/sim3.h:144-146,233-236.
//   E-7  operator*: r = r * o.r, t = s * (r * o.t) + t, s = s * o.s (sim3.h:266-272).
//   E-8  constructQuadraticForm (G/core/base_binary_edge.hpp:55-120): the information matrix is I * invSigma2, so
//        J^T (rho1 Omega) J is formed with one scalar w = rho1 * invSigma2 as (J_0i w) J_0j + (J_1i w) J_1j, and b from
//        omega_r = -(invSigma2 * e) * rho1 as J_0i r_0 + J_1i r_1; an edge's e12 term is added before its e21 term.
//   E-9  pow(2 rho - 1, 3) is the product (2 rho - 1)(2 rho - 1)(2 rho - 1); exp / sin / cos are the device library's.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "wave.hpp"
#include "lm_block.hpp"
#include "se3.hpp"
#include "sim3_math.hpp"

using orbg::block_sum;
using orbg::lane_ldlt_solve;
using orbg::select_device;
using orbg::wave_sum_f64;
using orbg_se3::quat_from_R;
using orbg_se3::quat_rotate;
using orbg_s3::S3;            // Sim3(Vector7d), operator*, inverse(): sim3_math.hpp
using orbg_s3::s3_exp;
using orbg_s3::s3_inverse;
using orbg_s3::s3_mul;

namespace {

constexpr int kS3oThreads = 256;
constexpr int kS3oTile = 1024;     // pairs staged in LDS: 12 floats each, 48 KiB
constexpr int kS3oNV = 36;         // 28 of H, 7 of b, chi2
constexpr int kS3oTrace = 15;      // 5 + 10 LM iterations at most

struct S3oDesc {                   // one problem of a launch
  int n, fix_scale, n_corr, pad;
  long long off_in;                // floats: X1 (3n) X2 (3n) obs1 (2n) obs2 (2n) w1 (n) w2 (n)
  long long off_chi;               // doubles: 4n -- chi2 of e12 / e21 as read at :4241, then as read at :4291
  long long off_rem;               // bytes: n
  double K1[4], K2[4];             // fx fy cx cy of pCamera1 / pCamera2 (float mvParameters promoted)
  double th2, delta;               // th2 and sqrt(th2), both floats in the reference, promoted
  S3 S;                            // g2oS12 on entry
};

struct S3oRec {                    // what the host reads back per problem
  int n_in, returned_early, n_bad1, trace_len, iters[2], pad[2];
  double chi2[2];
  S3 S;
  double trace[kS3oTrace][4];      // per LM iteration: round, lambda, chi2, trials
};

// VertexSim3Expmap::oplusImpl, I/OptimizableTypes.h:158-167, followed by the inverse every EdgeInverseSim3ProjectXYZ takes:
// E[0..8) = Sim3(update) * est, E[8..16) = its inverse, each as q[4] t[3] s
__device__ inline void s3o_oplus(const S3& est, const double* u, bool with_update, double* E) {
  S3 e = est, inv;
  if (with_update) {
    S3 ex;
    s3_exp(u, &ex);
    s3_mul(ex, est, &e);
  }
  s3_inverse(e, &inv);
#pragma unroll
  for (int k = 0; k < 4; k++) { E[k] = e.q[k]; E[8 + k] = inv.q[k]; }
#pragma unroll
  for (int k = 0; k < 3; k++) { E[4 + k] = e.t[k]; E[12 + k] = inv.t[k]; }
  E[7] = e.s; E[15] = inv.s;
}

struct S3oPair { double X1[3], X2[3], o1[2], o2[2], w1, w2; };

__device__ __forceinline__ void s3o_load(const float* in, int n, int i, S3oPair* P) {
  const size_t sn = (size_t)n, si = (size_t)i;
#pragma unroll
  for (int k = 0; k < 3; k++) { P->X1[k] = (double)in[3 * si + k]; P->X2[k] = (double)in[3 * sn + 3 * si + k]; }
#pragma unroll
  for (int k = 0; k < 2; k++) { P->o1[k] = (double)in[6 * sn + 2 * si + k]; P->o2[k] = (double)in[8 * sn + 2 * si + k]; }
  P->w1 = (double)in[10 * sn + si]; P->w2 = (double)in[11 * sn + si];
}

// the two computeError (I/OptimizableTypes.h:183-190, 204-211) with Pinhole::project(Eigen::Vector3d) (S/CameraModels/Pinhole.cpp:41-47:
// fx * x / z + cx, left to right) -> e[0..1] = e12, e[2..3] = e21
__device__ __forceinline__ void s3o_err(const double* E, const S3oPair& P, const double* K1, const double* K2, double* e) {
  double r[3];
  quat_rotate(E, P.X2, r);
  const double a0 = E[7] * r[0] + E[4], a1 = E[7] * r[1] + E[5], a2 = E[7] * r[2] + E[6];
  e[0] = P.o1[0] - (K1[0] * a0 / a2 + K1[2]);
  e[1] = P.o1[1] - (K1[1] * a1 / a2 + K1[3]);
  quat_rotate(E + 8, P.X1, r);
  const double b0 = E[15] * r[0] + E[12], b1 = E[15] * r[1] + E[13], b2 = E[15] * r[2] + E[14];
  e[2] = P.o2[0] - (K2[0] * b0 / b2 + K2[2]);
  e[3] = P.o2[1] - (K2[1] * b1 / b2 + K2[3]);
}

// RobustKernelHuber::robustify, G/core/robust_kernel_impl.cpp:78-91: rho[0], rho[1] (a NaN takes the else branch, as there)
__device__ __forceinline__ void s3o_huber(bool robust, double e, double delta, double dsqr, double* rho0, double* rho1) {
  if (!robust || e <= dsqr) { *rho0 = e; *rho1 = 1.0; }
  else { const double sq = sqrt(e); *rho0 = 2 * sq * delta - dsqr; *rho1 = delta / sq; }
}

template <bool LDS_IN>      // LDS_IN: n <= kS3oTile, `in` points into LDS (typed accesses; a pointer that may be either is a flat load)
__device__ __forceinline__ void s3o_run(const S3oDesc& D, const float* in, double* __restrict__ chi, uint8_t* __restrict__ rem, S3oRec* __restrict__ rec,
                        double (*s_est)[16], double (*s_part)[kS3oNV], double* s_tot, double (*s_wsum)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = min(lane, 6);
  const int n = D.n;
  const bool fix = D.fix_scale != 0;
  const double delta = D.delta, dsqr = delta * delta, th2 = D.th2;
  const double K1[4] = {D.K1[0], D.K1[1], D.K1[2], D.K1[3]}, K2[4] = {D.K2[0], D.K2[1], D.K2[2], D.K2[3]};
  const double kDelta = 1e-9, kScalar = 1.0 / (2 * kDelta);      // base_binary_edge.hpp:147-148
  S3 est = D.S;
  double x[7] = {0, 0, 0, 0, 0, 0, 0};
  int sum_slot = 0;
  for (int i = tid; i < n; i += kS3oThreads) { rem[i] = 0; chi[2 * (size_t)n + i] = 0; chi[3 * (size_t)n + i] = 0; }
  int nBad = 0, nIn = 0, trace_len = 0;
  int iters[2] = {0, 0};
  double chis[2] = {0, 0};
  bool early = false, robust = true;
  for (int round = 0; round < 2; round++) {
    double* const cs1 = chi + (round ? 2 * (size_t)n : 0);
    double* const cs2 = cs1 + n;
    const int its = round == 0 ? 5 : (nBad > 0 ? 10 : 5);                    // :4229, :4265-4269
    bool go = n - nBad > 0;                                                  // no active edge: optimize() returns at once
    double lambda = 0, ni = 2, cur = 0;
    int nBadLM = 0, done = 0;
    for (int it = 0; it < its && go; it++) {
      // ---- the estimate and its 14 perturbations, with their inverses: lanes 0..14, once per linearisation
      if (tid < 15) {
        const int d = (tid - 1) >> 1;
        const double dv = ((tid - 1) & 1) ? -kDelta : kDelta;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = (tid > 0 && k == d) ? dv : 0.0;
        if (fix) u[6] = 0;
        double E[16];
        s3o_oplus(est, u, tid > 0, E);
#pragma unroll
        for (int k = 0; k < 16; k++) s_est[tid][k] = E[k];
      }
      __syncthreads();
      // ---- computeActiveErrors + buildSystem at est
      double acc[kS3oNV];
#pragma unroll
      for (int k = 0; k < kS3oNV; k++) acc[k] = 0;
      for (int i = tid; i < n; i += kS3oThreads) {
        if (rem[i]) continue;
        S3oPair P;
        s3o_load(in, n, i, &P);
        double e0[4];
        s3o_err(s_est[0], P, K1, K2, e0);
        const double c1 = e0[0] * (P.w1 * e0[0]) + e0[1] * (P.w1 * e0[1]);   // BaseEdge::chi2(): _error.dot(information() * _error)
        const double c2 = e0[2] * (P.w2 * e0[2]) + e0[3] * (P.w2 * e0[3]);
        cs1[i] = c1; cs2[i] = c2;
        double r01, r11, r02, r12;
        s3o_huber(robust, c1, delta, dsqr, &r01, &r11);
        s3o_huber(robust, c2, delta, dsqr, &r02, &r12);
        acc[35] += r01; acc[35] += r02;
        double J[4][7];
#pragma unroll
        for (int d = 0; d < 7; d++) {
          // (the estimates are re-read from LDS for every pair: hoisted out of the pair loop they are 240 doubles per lane and the
          // kernel spills; the clobber keeps the loads where they are used)
          asm volatile("" ::: "memory");
          double ep[4], em[4];
          s3o_err(s_est[1 + 2 * d], P, K1, K2, ep);
          s3o_err(s_est[2 + 2 * d], P, K1, K2, em);
#pragma unroll
          for (int k = 0; k < 4; k++) J[k][d] = kScalar * (ep[k] - em[k]);
        }
        const double wo1 = r11 * P.w1, wo2 = r12 * P.w2;                     // robustInformation: rho[1] * information
        const double q10 = -(P.w1 * e0[0]) * r11, q11 = -(P.w1 * e0[1]) * r11;   // omega_r = -omega * _error; omega_r *= rho[1]
        const double q20 = -(P.w2 * e0[2]) * r12, q21 = -(P.w2 * e0[3]) * r12;
        int o = 0;
#pragma unroll
        for (int a = 0; a < 7; a++)
#pragma unroll
          for (int c = a; c < 7; c++) {
            acc[o] += (J[0][a] * wo1) * J[0][c] + (J[1][a] * wo1) * J[1][c];
            acc[o] += (J[2][a] * wo2) * J[2][c] + (J[3][a] * wo2) * J[3][c];
            o++;
          }
#pragma unroll
        for (int a = 0; a < 7; a++) {
          acc[28 + a] += J[0][a] * q10 + J[1][a] * q11;
          acc[28 + a] += J[2][a] * q20 + J[3][a] * q21;
        }
      }
      // ---- block sums in a fixed order
#pragma unroll
      for (int k = 0; k < kS3oNV; k++) {
        const double w = wave_sum_f64(acc[k]);
        if (lane == 0) s_part[wave][k] = w;
      }
      __syncthreads();
      if (tid < kS3oNV) s_tot[tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
      __syncthreads();
      // every thread takes its own copy of the system: row li of H (upper triangle packed row-major in s_tot[0..28)), b
      double Hrow[7], b[7];
#pragma unroll
      for (int j = 0; j < 7; j++) {
        const int a = min(li, j), c = max(li, j);
        Hrow[j] = s_tot[a * 7 - (a * (a - 1)) / 2 + (c - a)];
        b[j] = s_tot[28 + j];
      }
      const double b_li = s_tot[28 + li];
      cur = s_tot[35];
      const double iniChi = cur;
      if (it == 0) {
        // computeLambdaInit, levenberg.cpp:171-185: std::max(fabs(h_jj), maxDiagonal) returns its FIRST argument unless it is smaller
        double md = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) { const double a = fabs(s_tot[j * 7 - (j * (j - 1)) / 2]); md = (a < md) ? md : a; }
        lambda = 1e-5 * md; ni = 2; nBadLM = 0;
      }
      double rho = 0;
      int qmax = 0;
      for (;;) {
        const bool ok2 = lane_ldlt_solve<7>(Hrow, b_li, li, lambda, x);
        if (fix) x[6] = 0;                                     // oplusImpl writes the zero into the solver's x
        double E[16];
        s3o_oplus(est, x, true, E);                            // update() runs also after a refused solve, with the x that is there
        double tchi = 0;
        // the errors of the LAST evaluation stay with the edges, accepted or not
        for (int i = tid; i < n; i += kS3oThreads) {
          if (rem[i]) continue;
          S3oPair P;
          s3o_load(in, n, i, &P);
          double e[4];
          s3o_err(E, P, K1, K2, e);
          const double c1 = e[0] * (P.w1 * e[0]) + e[1] * (P.w1 * e[1]);
          const double c2 = e[2] * (P.w2 * e[2]) + e[3] * (P.w2 * e[3]);
          cs1[i] = c1; cs2[i] = c2;
          double r0, r1;
          s3o_huber(robust, c1, delta, dsqr, &r0, &r1); tchi += r0;
          s3o_huber(robust, c2, delta, dsqr, &r0, &r1); tchi += r0;
        }
        double tempChi = block_sum(tchi, s_wsum, sum_slot); sum_slot ^= 1;
        if (!ok2) tempChi = 1.7976931348623157e308;
        rho = cur - tempChi;
        double scale = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
        scale += 1e-3;
        rho /= scale;
        if (rho > 0 && fabs(tempChi) != INFINITY && tempChi == tempChi) {
          double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
          alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;         // std::min(alpha, _goodStepUpperScale)
          const double sf = (1. / 3. < alpha) ? alpha : 1. / 3.;   // std::max(_goodStepLowerScale, alpha)
          lambda *= sf;
          ni = 2;
          cur = tempChi;
#pragma unroll
          for (int k = 0; k < 4; k++) est.q[k] = E[k];
#pragma unroll
          for (int k = 0; k < 3; k++) est.t[k] = E[4 + k];
          est.s = E[7];
        } else {
          lambda *= ni; ni *= 2;
        }
        qmax++;
        if (!(rho < 0 && qmax < 10)) break;
      }
      if (tid == 0 && trace_len < kS3oTrace) {
        rec->trace[trace_len][0] = round; rec->trace[trace_len][1] = lambda; rec->trace[trace_len][2] = cur; rec->trace[trace_len][3] = qmax;
      }
      trace_len++;
      done++;
      if (qmax == 10 || rho == 0) go = false;
      else {
        if ((iniChi - cur) * 1e3 < iniChi) nBadLM++; else nBadLM = 0;
        if (nBadLM >= 3) go = false;
      }
      __syncthreads();                                         // s_est / s_part / s_tot are rewritten by the next linearisation
    }
    iters[round] = done; chis[round] = cur;
    if (round == 0) {
      // :4234-4261 -- chi2() as the last evaluation left it
      double bl = 0;
      for (int i = tid; i < n; i += kS3oThreads) {
        const bool bad = cs1[i] > th2 || cs2[i] > th2;
        if (bad) { rem[i] = 1; bl += 1; }
      }
      nBad = (int)block_sum(bl, s_wsum, sum_slot); sum_slot ^= 1;
      robust = false;                                          // setRobustKernel(0)
      if (D.n_corr - nBad < 10) { early = true; break; }       // :4271
    } else {
      // :4281-4301 -- computeError, then the same test
      double E[16];
      s3o_oplus(est, x, false, E);
      double cnt = 0;
      for (int i = tid; i < n; i += kS3oThreads) {
        if (rem[i]) continue;
        S3oPair P;
        s3o_load(in, n, i, &P);
        double e[4];
        s3o_err(E, P, K1, K2, e);
        const double c1 = e[0] * (P.w1 * e[0]) + e[1] * (P.w1 * e[1]);
        const double c2 = e[2] * (P.w2 * e[2]) + e[3] * (P.w2 * e[3]);
        cs1[i] = c1; cs2[i] = c2;
        if (c1 > th2 || c2 > th2) rem[i] = 2; else cnt += 1;
      }
      nIn = (int)block_sum(cnt, s_wsum, sum_slot); sum_slot ^= 1;
    }
  }
  if (tid == 0) {
    rec->n_in = nIn; rec->returned_early = early ? 1 : 0; rec->n_bad1 = nBad; rec->trace_len = min(trace_len, kS3oTrace);
    rec->iters[0] = iters[0]; rec->iters[1] = iters[1]; rec->pad[0] = 0; rec->pad[1] = 0;
    rec->chi2[0] = chis[0]; rec->chi2[1] = chis[1];
    rec->S = early ? D.S : est;                                // the early return does not write g2oS12
  }
}

__global__ __launch_bounds__(kS3oThreads) void sim3_opt_kernel(const S3oDesc* __restrict__ descs, const float* __restrict__ inputs,
                                                              double* __restrict__ chi, uint8_t* __restrict__ rem, S3oRec* __restrict__ recs) {
  __shared__ float s_in[12 * kS3oTile];
  __shared__ double s_est[15][16];
  __shared__ double s_part[4][kS3oNV];
  __shared__ double s_tot[kS3oNV];
  __shared__ double s_wsum[2][4];
  const S3oDesc D = descs[blockIdx.x];
  const float* gin = inputs + D.off_in;
  if (D.n <= kS3oTile) {
    for (int i = threadIdx.x; i < 12 * D.n; i += kS3oThreads) s_in[i] = gin[i];
    __syncthreads();
    s3o_run<true>(D, s_in, chi + D.off_chi, rem + D.off_rem, recs + blockIdx.x, s_est, s_part, s_tot, s_wsum);
  } else {
    s3o_run<false>(D, gin, chi + D.off_chi, rem + D.off_rem, recs + blockIdx.x, s_est, s_part, s_tot, s_wsum);
  }
}

// ------------------------------------------------------------------------------------------------ host side

struct S3oBufs {                 // the calling thread's buffers: one staging block (inputs up, records down) and the per-edge chi2
  orbg::StageBlock blk;
  orbg::DevBuf<double> d_chi;
  std::vector<double> h_chi;
  void release_buffers() { blk.release(); d_chi.release(); }
};
using S3oWork = orbg::WorkArea<S3oBufs>;
S3oWork& s3o_work() { static thread_local S3oWork w; return w; }

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
  return true;
}

int check_problem(const orbm_sim3opt_problem* p) {
  if (!p || p->struct_size < sizeof(orbm_sim3opt_problem) || p->n < 0) return ORBG_BAD_ARG;
  if (p->n > 0 && (!p->X3Dc1 || !p->X3Dc2 || !p->obs1 || !p->obs2 || !p->inv_sigma2_1 || !p->inv_sigma2_2)) return ORBG_BAD_ARG;
  if (p->camera_model1 != 0 || p->camera_model2 != 0) return ORBG_BAD_ARG;      // pinhole only: nothing else is approximated
  if (!finite_all(p->q, 4) || !finite_all(p->t, 3) || !std::isfinite(p->s)) return ORBG_BAD_ARG;
  if (!(p->th2 > 0.0f)) return ORBG_BAD_ARG;
  return ORBG_OK;
}

}  // namespace

extern "C" int orbm_sim3_optimize_batch(int device, const orbm_sim3opt_problem* problems, int B, orbm_sim3opt_result* results) {
  if (B < 0 || (B > 0 && (!problems || !results))) return ORBG_BAD_ARG;
  // every argument is checked, and the device, before any result is written: a call that fails leaves `results` as it found them
  int rc;
  for (int b = 0; b < B; b++) {
    if ((rc = check_problem(&problems[b]))) return rc;
    if (results[b].struct_size < sizeof(orbm_sim3opt_result)) return ORBG_BAD_ARG;
    if (results[b].trace_cap < 0 || (results[b].trace_cap > 0 && !results[b].trace)) return ORBG_BAD_ARG;
  }
  if ((rc = select_device(device))) return rc;
  std::vector<int> job_of(B, -1);
  std::vector<int> jobs;
  size_t n_tot = 0;
  bool want_chi = false;
  for (int b = 0; b < B; b++) {
    if (problems[b].n == 0) continue;                        // an empty graph: optimize() does nothing, 0 - 0 < 10 -> return 0, no launch
    job_of[b] = (int)jobs.size();
    jobs.push_back(b);
    n_tot += (size_t)problems[b].n;
    want_chi = want_chi || results[b].edge_chi2;
  }
  const int J = (int)jobs.size();
  S3oWork* w = nullptr;
  const S3oRec* recs = nullptr;
  const uint8_t* rems = nullptr;
  std::vector<S3oDesc> descs(J);
  if (J > 0) {
    w = &s3o_work();
    if ((rc = w->open(device, "misc"))) return rc;
    orbg::StageBlock& S = w->blk;
    orbg::StageLayout lay;
    const auto s_desc = lay.add<S3oDesc>(J);               // in: one upload over the first two slots
    const auto s_in = lay.add<float>(12 * n_tot);
    const auto s_rec = lay.add<S3oRec>(J);                 // out: one download over the last two
    const auto s_rem = lay.add<uint8_t>(n_tot);
    if ((rc = S.reserve(lay.bytes())) || (rc = w->d_chi.reserve(4 * n_tot))) return rc;
    float* hin = S.host(s_in);
    size_t off = 0;
    for (int j = 0; j < J; j++) {
      const orbm_sim3opt_problem& p = problems[jobs[j]];
      const size_t n = (size_t)p.n;
      S3oDesc& D = descs[j];
      memset(&D, 0, sizeof(D));
      D.n = p.n; D.fix_scale = p.fix_scale ? 1 : 0; D.n_corr = p.n_correspondences;
      D.off_in = (long long)(12 * off); D.off_chi = (long long)(4 * off); D.off_rem = (long long)off;
      D.K1[0] = p.fx1; D.K1[1] = p.fy1; D.K1[2] = p.cx1; D.K1[3] = p.cy1;
      D.K2[0] = p.fx2; D.K2[1] = p.fy2; D.K2[2] = p.cx2; D.K2[3] = p.cy2;
      D.th2 = (double)p.th2;
      D.delta = (double)sqrtf(p.th2);                        // const float deltaHuber = sqrt(th2), :4073
      for (int k = 0; k < 4; k++) D.S.q[k] = p.q[k];
      for (int k = 0; k < 3; k++) D.S.t[k] = p.t[k];
      D.S.s = p.s;
      float* dst = hin + 12 * off;
      memcpy(dst, p.X3Dc1, 12 * n); memcpy(dst + 3 * n, p.X3Dc2, 12 * n);
      memcpy(dst + 6 * n, p.obs1, 8 * n); memcpy(dst + 8 * n, p.obs2, 8 * n);
      memcpy(dst + 10 * n, p.inv_sigma2_1, 4 * n); memcpy(dst + 11 * n, p.inv_sigma2_2, 4 * n);
      off += n;
    }
    S.put(s_desc, descs.data());
    hipStream_t st = w->stream;
    if ((rc = S.upload(s_desc.off, s_in.end(), st))) return rc;
    hipLaunchKernelGGL(sim3_opt_kernel, dim3(J), dim3(kS3oThreads), 0, st, (const S3oDesc*)S.device(s_desc), (const float*)S.device(s_in),
                       w->d_chi.p, S.device(s_rem), S.device(s_rec));
    ORBG_HIP(hipGetLastError());
    if ((rc = S.download(s_rec.off, s_rem.end(), st))) return rc;
    if (want_chi) {
      w->h_chi.resize(4 * n_tot);
      ORBG_HIP(hipMemcpyAsync(w->h_chi.data(), w->d_chi.p, 4 * n_tot * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    ORBG_HIP(hipStreamSynchronize(st));
    recs = S.host(s_rec);
    rems = S.host(s_rem);
  }
  for (int b = 0; b < B; b++) {
    const orbm_sim3opt_problem& p = problems[b];
    orbm_sim3opt_result* r = &results[b];
    r->trace_len = 0;
    if (job_of[b] < 0) {
      r->n_in = 0; r->returned_early = 1; r->n_bad_round1 = 0;
      for (int k = 0; k < 4; k++) r->q[k] = p.q[k];
      for (int k = 0; k < 3; k++) r->t[k] = p.t[k];
      r->s = p.s;
      r->iters[0] = r->iters[1] = 0; r->chi2[0] = r->chi2[1] = 0;
      continue;
    }
    const S3oRec& rec = recs[job_of[b]];
    const S3oDesc& D = descs[job_of[b]];
    const size_t n = (size_t)p.n;
    r->n_in = rec.n_in; r->returned_early = rec.returned_early; r->n_bad_round1 = rec.n_bad1;
    for (int k = 0; k < 4; k++) r->q[k] = rec.S.q[k];
    for (int k = 0; k < 3; k++) r->t[k] = rec.S.t[k];
    r->s = rec.S.s;
    r->iters[0] = rec.iters[0]; r->iters[1] = rec.iters[1]; r->chi2[0] = rec.chi2[0]; r->chi2[1] = rec.chi2[1];
    if (r->removed) memcpy(r->removed, rems + D.off_rem, n);
    if (r->trace) {
      r->trace_len = std::min(rec.trace_len, r->trace_cap);
      memcpy(r->trace, rec.trace, (size_t)r->trace_len * 4 * sizeof(double));
    }
    if (r->edge_chi2) memcpy(r->edge_chi2, w->h_chi.data() + D.off_chi, 4 * n * sizeof(double));
  }
  return ORBG_OK;
}

extern "C" int orbm_sim3_optimize(int device, const orbm_sim3opt_problem* p, orbm_sim3opt_result* r) {
  if (!p || !r) return ORBG_BAD_ARG;
  return orbm_sim3_optimize_batch(device, p, 1, r);
}
