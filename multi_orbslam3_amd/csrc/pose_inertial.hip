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
// All of it in double.  Every sum has a fixed order: the result is bit-reproducible from run to run.  The Huber
// kernel is lm_step.hpp's (through pi_huber); the word that completes the launch is common.hpp's SolveWord.
namespace {

constexpr int kPiThreads = 256;
constexpr int kPiMaxN = 4096;

// the vertices and the edge arithmetic (PiState, PiParams, kPiLd, pi_*): shared with the local inertial BA
#include "pose_inertial_edges.hpp"

// what the kernel leaves in the staging block next to the outlier flags; stats: nBad, rounds run, solve failed, .., [7] = the
// sequence number that completes the record
struct PiOut { PiState cur; double chi2[4]; double H[900]; int stats[8]; };

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
  solve_word_complete(&out->stats[7], seq);
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
  static thread_local orbg::SolveWord done_word;
  PiOut* ho = S.host(s_out);
  const unsigned pi_seq = done_word.arm(&ho->stats[7]);
  if (p->form == POSE_INERTIAL_LAST_FRAME)
    hipLaunchKernelGGL(pose_inertial_kernel<30>, dim3(1), dim3(kPiThreads), 0, sc.stream, (const PiParams*)S.device(s_prm), dX, du, dv, dur, dom, dcl,
                       S.mapped(s_out), S.mapped(s_flag), pi_seq);
  else
    hipLaunchKernelGGL(pose_inertial_kernel<15>, dim3(1), dim3(kPiThreads), 0, sc.stream, (const PiParams*)S.device(s_prm), dX, du, dv, dur, dom, dcl,
                       S.mapped(s_out), S.mapped(s_flag), pi_seq);
  ORBG_HIP(hipGetLastError());
  if ((rc = done_word.wait(sc.stream))) return rc;
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
