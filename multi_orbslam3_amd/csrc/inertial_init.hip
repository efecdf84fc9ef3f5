// liborbgpu -- Optimizer::InertialOptimization for gfx950 (MI355X): the IMU initialisation of an inertial agent, the whole optimize() in
// one kernel launch (include/orbgpu.h: inertial_init_solve).
#include <time.h>

#include <cmath>
#include <vector>

#include "common.hpp"
#include "wave.hpp"
#include "lm_block.hpp"

using namespace orbg;

// ------------------------------------------------------------------------------------------------
// S/Optimizer.cc:5344-5958, four overloads of one graph: every pose fixed, one EdgeInertialGS (S/G2oTypes.cc:802-927) per keyframe with
// an mPrevKF, one gyro bias, one accelerometer bias, the gravity direction and the scale shared by all edges, two prior edges on the
// biases.  The overloads differ in what is free, in the algorithm (g2o's Levenberg-Marquardt with ORB-SLAM3's _nBad rule, or
// Gauss-Newton) and in the iteration count: the problem says which.
//
// The system has 3 Nv + 9 unknowns at most: a 3 x 3 block per velocity, an off-diagonal block only between a keyframe and its
// predecessor, and a border of up to 9 columns (bg, ba, gdir, s) that every edge touches.  It is never formed densely.  The predecessor
// relation is a forest, so eliminating every velocity after all of its successors causes no fill: the host computes that order once
// per call, the kernel keeps per vertex D (6), O toward the predecessor (9), B toward the border (3 x 9) and b (3), and the 9 x 9 corner.
// A column whose vertex is fixed is not a variable: nothing is computed for it.
//
// One 256-thread workgroup.  Per iteration:
//   1. thread t linearises edges t, t + 256, ...: the 9 x 16 block J (pi_inertial_gs_edge) and the upper triangle of J^T W J (136 values per
//      edge, work area); the corner, its right-hand side and chi2 are summed over the edges: tree sums inside a wavefront, then the four
//      wavefronts in order;
//   and per trial (one per Gauss-Newton iteration, up to ten per LM iteration):
//   2. thread t gathers the blocks of vertices t, t + 256, ... from the edge blocks: the incoming edge, then the outgoing edges in edge
//      order (no atomics);
//   3. wavefront 0 walks the elimination order: (D + lambda I)^-1 by cofactors, lanes 0..35 subtract the step's term from the
//      predecessor's D, B and b;
//   4. the Schur terms B^T (D + lambda I)^-1 [B b] of all vertices are summed as in 1. and subtracted from the corner, which
//      wavefront 0 solves (lane_ldlt_solve, 9 wide; a fixed border column is an identity row);
//   5. back-substitution: c = D^-1 (b - B x_border) and N = D^-1 O per vertex in parallel, then x = c - N x_pred along the reverse order;
//   6. the trial state, its chi2 (summed as in 1.), g2o's verdict.
// Up to kIiTile keyframes the per-vertex blocks live in LDS, beyond that in the calling thread's work area.  Everything in double
// (DESIGN section 5); every sum has a fixed order: two calls on the same input return the same bits.
//
// One deviation, the one pose_inertial_optimize documents: a pivot that is not positive and finite refuses the solve.  Under LM the trial
// counts as failed (lm_trial_verdict); under Gauss-Newton no update is applied, solve_failed is set and the run ends (the reference applies
// an undefined update there).  Under Gauss-Newton a corner pivot no larger than 2^-40 of its own diagonal entry counts as not positive
// (lane_ldlt_solve's REL form).
namespace {

constexpr int kIiThreads = 256;
constexpr int kIiTile = 256;       // keyframes whose per-vertex blocks live in LDS (kIiVtx doubles each: 102 KiB of the CU's 160)
constexpr int kIiVtx = 51;         // D 6 | O 9 | B 27 | b 3 | the b of the linearisation 3 | x 3; odd: consecutive vertices start in different banks
constexpr int kIiJ = 9 * 16;       // an edge's block [v1 | v2 | bg | ba | gdir | s | e]
constexpr int kIiH = 136;          // the upper triangle of its 16 x 16 J^T W J
constexpr int kIiNV = 55;          // the corner's upper triangle (45), its right-hand side (9), chi2
enum { kVD = 0, kVO = 6, kVB = 15, kVb = 42, kVb0 = 45, kVx = 48 };

// the vertices and the edge arithmetic (PiGsEdge, pi_inertial_gs_edge, pi_gdir_oplus): shared with the other inertial optimisers
#include "pose_inertial_edges.hpp"

struct IiBorder { double bg[3], ba[3], Rwg[9], s; };
struct IiParams {
  int nk, ne, nv, algorithm, iterations, groups, priors, trace_cap;
  double lambda_init, prior_g, prior_a;
  IiBorder start;
};
struct IiKf { double R[9], t[3]; };
// what the kernel leaves in the staging block; seq completes the record
struct IiOut { IiBorder end; double chi2_first, chi2_final; int iters, solve_failed, trace_len, seq; };

__host__ __device__ constexpr int ii_tri16(int a, int c) { return a * 16 - (a * (a - 1)) / 2 + (c - a); }     // a <= c
__host__ __device__ constexpr int ii_tri9(int a, int c) { return a * 9 - (a * (a - 1)) / 2 + (c - a); }

// the columns of an edge's block that are variables: bit c of the result
__host__ __device__ inline int ii_column_mask(int groups) {
  return ((groups & kGsVel) ? 0x3F : 0) | ((groups & kGsBias) ? 0xFC0 : 0) | ((groups & kGsGdir) ? 0x3000 : 0) | ((groups & kGsScale) ? 0x4000 : 0) | 0x8000;
}

template <bool kLds>      // kLds: nk <= kIiTile, the per-vertex blocks are in LDS (typed accesses; a pointer that may be either is a flat load)
__global__ __launch_bounds__(kIiThreads) void inertial_init_kernel(const IiParams* __restrict__ gP, const IiKf* __restrict__ kf, const PiGsEdge* __restrict__ ed,
                                                                  const double* __restrict__ v0, const int* __restrict__ order,
                                                                  const int* __restrict__ pred, const int* __restrict__ in_edge,
                                                                  const int* __restrict__ out_start, const int* __restrict__ out_edge, double* Jbuf,
                                                                  double* Hbuf, double* Vglob, double* vcur, double* vtrial, IiOut* __restrict__ out,
                                                                  double* __restrict__ vout, double* __restrict__ trace, unsigned seq) {
  __shared__ double s_V[kLds ? kIiTile * kIiVtx : 1];
  __shared__ IiParams P;
  __shared__ IiBorder s_cur, s_trial;
  __shared__ double s_part[4][kIiNV + 1], s_tot[kIiNV + 1];
  __shared__ double s_C[81], s_C2[81], s_rhs0[9], s_rhs[9], s_xb[9];
  __shared__ double s_wsum[2][4], s_max[kIiThreads];
  __shared__ int s_ok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int sum_slot = 0;
  {
    const double* src = reinterpret_cast<const double*>(gP);
    double* dst = reinterpret_cast<double*>(&P);
    for (int i = tid; i < (int)(sizeof(IiParams) / sizeof(double)); i += kIiThreads) dst[i] = src[i];
  }
  __syncthreads();
  const int nk = P.nk, ne = P.ne, nv = P.nv, groups = P.groups;
  const int colmask = ii_column_mask(groups), bmask = (colmask >> 6) & 0x1FF;       // bmask: the free border columns
  const bool priors = P.priors != 0, gn = P.algorithm == INERTIAL_INIT_GN;
  double* V;
  if constexpr (kLds) V = s_V; else V = Vglob;
  for (int i = tid; i < 3 * nk; i += kIiThreads) vcur[i] = v0[i];
  if (tid == 0) s_cur = P.start;
  __syncthreads();

  // block sums of acc[0..kIiNV) in a fixed order -> s_tot
  auto reduce = [&](const double* acc) {
#pragma unroll
    for (int k = 0; k < kIiNV; k++) {
      const double w = wave_sum_f64(acc[k]);
      if (lane == 0) s_part[wave][k] = w;
    }
    __syncthreads();
    if (tid < kIiNV) s_tot[tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
    __syncthreads();
  };
  // the chi2 of the prior edges (EdgePriorAcc, EdgePriorGyro, I/G2oTypes.h:784-830: error = 0 - bias) at a border state
  auto prior_chi2 = [&](const IiBorder& b) -> double {
    double c = 0;
    if (priors) {
#pragma unroll
      for (int i = 0; i < 3; i++) c += b.ba[i] * (P.prior_a * b.ba[i]);
#pragma unroll
      for (int i = 0; i < 3; i++) c += b.bg[i] * (P.prior_g * b.bg[i]);
    }
    return c;
  };

  // step 1 at the current estimate: the edge blocks, the corner s_C / s_rhs0; returns chi2
  auto linearise = [&]() -> double {
    double acc[kIiNV];
#pragma unroll
    for (int k = 0; k < kIiNV; k++) acc[k] = 0;
    for (int e = tid; e < ne; e += kIiThreads) {
      const PiGsEdge& E = ed[e];
      double* J = Jbuf + (size_t)e * kIiJ;
      double* H = Hbuf + (size_t)e * kIiH;
      pi_inertial_gs_edge(E, kf[E.k1].R, kf[E.k1].t, vcur + 3 * E.k1, kf[E.k2].R, kf[E.k2].t, vcur + 3 * E.k2, s_cur.bg, s_cur.ba, s_cur.Rwg, s_cur.s,
                          groups, J);
#pragma unroll 1
      for (int c = 0; c < 16; c++) {
        if (!((colmask >> c) & 1)) continue;
        double jc[9], wj[9];
#pragma unroll
        for (int r = 0; r < 9; r++) jc[r] = J[r * kGsLd + c];
#pragma unroll
        for (int r = 0; r < 9; r++) {
          double s = 0;
#pragma unroll
          for (int k = 0; k < 9; k++) s += E.info9[9 * r + k] * jc[k];
          wj[r] = s;
        }
#pragma unroll 1
        for (int a = 0; a <= c; a++) {
          if (!((colmask >> a) & 1)) continue;
          double s = 0;
#pragma unroll
          for (int r = 0; r < 9; r++) s += J[r * kGsLd + a] * wj[r];
          H[ii_tri16(a, c)] = s;
        }
      }
#pragma unroll
      for (int a = 0; a < 9; a++) {
        if (!((bmask >> a) & 1)) continue;
#pragma unroll
        for (int c = a; c < 9; c++)
          if ((bmask >> c) & 1) acc[ii_tri9(a, c)] += H[ii_tri16(kGsColBg + a, kGsColBg + c)];
        acc[45 + a] -= H[ii_tri16(kGsColBg + a, kGsColE)];
      }
      acc[54] += H[ii_tri16(kGsColE, kGsColE)];
    }
    reduce(acc);
    if (tid < 81) {
      const int a = tid / 9, c = tid % 9;
      double h = a == c ? 1.0 : 0.0;                       // a fixed border column: an identity row of the 9-wide solve
      if (((bmask >> a) & 1) && ((bmask >> c) & 1)) {
        h = s_tot[ii_tri9(min(a, c), max(a, c))];
        if (priors && a == c && a < 6) h += a < 3 ? P.prior_g : P.prior_a;
      }
      s_C[tid] = h;
    }
    if (tid < 9) {
      double r = 0;
      if ((bmask >> tid) & 1) {
        r = s_tot[45 + tid];
        // the prior edges' linearizeOplus is +I on an error of -bias (S/G2oTypes.cc:971-983): b = -J^T W e = +prior * bias
        if (priors && tid < 6) r += tid < 3 ? P.prior_g * s_cur.bg[tid] : P.prior_a * s_cur.ba[tid - 3];
      }
      s_rhs0[tid] = r;
    }
    const double chi = s_tot[54] + prior_chi2(s_cur);
    __syncthreads();
    return chi;
  };

  // step 2: the per-vertex blocks of this linearisation
  auto gather = [&]() {
    if (!(groups & kGsVel)) return;
    for (int idx = tid; idx < nv; idx += kIiThreads) {
      const int k = order[idx];
      double* Vk = V + (size_t)k * kIiVtx;
      double D[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
      const int ei = in_edge[k];
      if (ei >= 0) {
        const double* H = Hbuf + (size_t)ei * kIiH;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = i; j < 3; j++) D[q++] += H[ii_tri16(kGsColV2 + i, kGsColV2 + j)];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
          for (int m = 0; m < 3; m++) Vk[kVO + 3 * i + m] = H[ii_tri16(kGsColV1 + m, kGsColV2 + i)];     // H(v_k row i, v_pred column m)
#pragma unroll
          for (int j = 0; j < 9; j++)
            if ((bmask >> j) & 1) Vk[kVB + 9 * i + j] = H[ii_tri16(kGsColV2 + i, kGsColBg + j)];
          b[i] -= H[ii_tri16(kGsColV2 + i, kGsColE)];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 9; j++)
            if ((bmask >> j) & 1) Vk[kVB + 9 * i + j] = 0;
      }
      for (int o = out_start[k]; o < out_start[k + 1]; o++) {
        const double* H = Hbuf + (size_t)out_edge[o] * kIiH;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = i; j < 3; j++) D[q++] += H[ii_tri16(kGsColV1 + i, kGsColV1 + j)];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
          for (int j = 0; j < 9; j++)
            if ((bmask >> j) & 1) Vk[kVB + 9 * i + j] += H[ii_tri16(kGsColV1 + i, kGsColBg + j)];
          b[i] -= H[ii_tri16(kGsColV1 + i, kGsColE)];
        }
      }
#pragma unroll
      for (int i = 0; i < 6; i++) Vk[kVD + i] = D[i];
#pragma unroll
      for (int i = 0; i < 3; i++) { Vk[kVb + i] = b[i]; Vk[kVb0 + i] = b[i]; }
    }
    __syncthreads();
  };

  // steps 3-5: (H + lambda I) x = b; x of the velocities -> the vertices' x slots, of the border -> s_xb.  False (for every thread) when a
  // pivot was refused.
  auto solve = [&](double lambda) -> bool {
    const bool vel = (groups & kGsVel) != 0;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    if (vel && wave == 0) {
      // the entry of the predecessor's blocks this lane updates: 0..5 D (upper triangle), 6..32 B, 33..35 b
      const int l = lane;
      int ei = 0, ej = 0;
      if (l < 6) { ei = l < 3 ? 0 : l < 5 ? 1 : 2; ej = l < 3 ? l : l < 5 ? l - 2 : 2; }
      else if (l < 33) { ei = (l - 6) / 9; ej = (l - 6) % 9; }
      else if (l < 36) ei = l - 33;
      const bool act = l < 6 || (l < 33 && ((bmask >> ej) & 1)) || (l >= 33 && l < 36);
      bool ok = true;
      for (int idx = 0; idx < nv; idx++) {
        const int k = order[idx], p = pred[k];
        double* Vk = V + (size_t)k * kIiVtx;
        const double a00 = Vk[0] + lambda, a01 = Vk[1], a02 = Vk[2], a11 = Vk[3] + lambda, a12 = Vk[4], a22 = Vk[5] + lambda;
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = a00 * c00 + a01 * c01 + a02 * c02;
        // the pivots of an LDL^T of this block are a00, c22 / a00 and det / c22
        if (!(a00 > 0.0) || !(c22 > 0.0) || !(det > 0.0) || fabs(det) == INFINITY) { ok = false; break; }
        const double M[9] = {c00 / det, c01 / det, c02 / det, c01 / det, c11 / det, c12 / det, c02 / det, c12 / det, c22 / det};
        if (l < 6) Vk[kVD + l] = M[3 * ei + ej];
        if (p >= 0 && act) {
          double* Vp = V + (size_t)p * kIiVtx;
          double G[3];                                     // row ei of O^T M
#pragma unroll
          for (int m = 0; m < 3; m++) G[m] = (Vk[kVO + ei] * M[m] + Vk[kVO + 3 + ei] * M[3 + m]) + Vk[kVO + 6 + ei] * M[6 + m];
          if (l < 6) Vp[kVD + l] -= (G[0] * Vk[kVO + ej] + G[1] * Vk[kVO + 3 + ej]) + G[2] * Vk[kVO + 6 + ej];
          else if (l < 33) Vp[kVB + 9 * ei + ej] -= (G[0] * Vk[kVB + ej] + G[1] * Vk[kVB + 9 + ej]) + G[2] * Vk[kVB + 18 + ej];
          else Vp[kVb + ei] -= (G[0] * Vk[kVb] + G[1] * Vk[kVb + 1]) + G[2] * Vk[kVb + 2];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // the next step reads what other lanes of this wavefront wrote
      }
      if (!ok && l == 0) s_ok = 0;
    }
    __syncthreads();
    if (!s_ok) return false;
    // step 4: the corner minus the Schur terms
    if (vel) {
      double acc[kIiNV];
#pragma unroll
      for (int k = 0; k < kIiNV; k++) acc[k] = 0;
      for (int idx = tid; idx < nv; idx += kIiThreads) {
        const double* Vk = V + (size_t)order[idx] * kIiVtx;
        const double M[9] = {Vk[0], Vk[1], Vk[2], Vk[1], Vk[3], Vk[4], Vk[2], Vk[4], Vk[5]};
        double Mb[3];
#pragma unroll
        for (int m = 0; m < 3; m++) Mb[m] = (M[3 * m] * Vk[kVb] + M[3 * m + 1] * Vk[kVb + 1]) + M[3 * m + 2] * Vk[kVb + 2];
#pragma unroll
        for (int c = 0; c < 9; c++) {
          if (!((bmask >> c) & 1)) continue;
          double MB[3];
#pragma unroll
          for (int m = 0; m < 3; m++) MB[m] = (M[3 * m] * Vk[kVB + c] + M[3 * m + 1] * Vk[kVB + 9 + c]) + M[3 * m + 2] * Vk[kVB + 18 + c];
#pragma unroll
          for (int a = 0; a <= c; a++)
            if ((bmask >> a) & 1) acc[ii_tri9(a, c)] += (Vk[kVB + a] * MB[0] + Vk[kVB + 9 + a] * MB[1]) + Vk[kVB + 18 + a] * MB[2];
          acc[45 + c] += (Vk[kVB + c] * Mb[0] + Vk[kVB + 9 + c] * Mb[1]) + Vk[kVB + 18 + c] * Mb[2];
        }
      }
      reduce(acc);
    }
    if (tid < 81) {
      const int a = tid / 9, c = tid % 9;
      double h = s_C[tid];
      if (vel && ((bmask >> a) & 1) && ((bmask >> c) & 1)) h -= s_tot[ii_tri9(min(a, c), max(a, c))];
      s_C2[tid] = h;
    }
    if (tid < 9) {
      double r = s_rhs0[tid];
      if (vel && ((bmask >> tid) & 1)) r -= s_tot[45 + tid];
      s_rhs[tid] = r;
      s_xb[tid] = 0;
    }
    __syncthreads();
    if (bmask && wave == 0) {
      const int li = min(lane, 8);
      double Hrow[9], x[9];
#pragma unroll
      for (int j = 0; j < 9; j++) { Hrow[j] = s_C2[9 * li + j]; x[j] = 0; }
      const bool ok = gn ? lane_ldlt_solve<9, true>(Hrow, s_rhs[li], li, lambda, x) : lane_ldlt_solve<9, false>(Hrow, s_rhs[li], li, lambda, x);
      if (lane == 0) {
        s_ok = ok ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 9; j++) s_xb[j] = ((bmask >> j) & 1) ? x[j] : 0.0;
      }
    }
    __syncthreads();
    if (!s_ok) return false;
    // step 5
    if (vel) {
      for (int idx = tid; idx < nv; idx += kIiThreads) {
        const int k = order[idx];
        double* Vk = V + (size_t)k * kIiVtx;
        const double M[9] = {Vk[0], Vk[1], Vk[2], Vk[1], Vk[3], Vk[4], Vk[2], Vk[4], Vk[5]};
        double r[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
          double s = Vk[kVb + m];
#pragma unroll
          for (int j = 0; j < 9; j++)
            if ((bmask >> j) & 1) s -= Vk[kVB + 9 * m + j] * s_xb[j];
          r[m] = s;
        }
        if (pred[k] >= 0) {
          double N[9];
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int m = 0; m < 3; m++) N[3 * i + m] = (M[3 * i] * Vk[kVO + m] + M[3 * i + 1] * Vk[kVO + 3 + m]) + M[3 * i + 2] * Vk[kVO + 6 + m];
#pragma unroll
          for (int i = 0; i < 9; i++) Vk[kVO + i] = N[i];
        }
#pragma unroll
        for (int m = 0; m < 3; m++) Vk[kVb + m] = (M[3 * m] * r[0] + M[3 * m + 1] * r[1]) + M[3 * m + 2] * r[2];
      }
      __syncthreads();
      if (tid == 0) {
        for (int idx = nv - 1; idx >= 0; idx--) {
          const int k = order[idx], p = pred[k];
          double* Vk = V + (size_t)k * kIiVtx;
          double x[3] = {Vk[kVb], Vk[kVb + 1], Vk[kVb + 2]};
          if (p >= 0) {
            const double* xp = V + (size_t)p * kIiVtx + kVx;
#pragma unroll
            for (int i = 0; i < 3; i++) x[i] -= (Vk[kVO + 3 * i] * xp[0] + Vk[kVO + 3 * i + 1] * xp[1]) + Vk[kVO + 3 * i + 2] * xp[2];
          }
#pragma unroll
          for (int i = 0; i < 3; i++) Vk[kVx + i] = x[i];
        }
      }
      __syncthreads();
    }
    return true;
  };

  // step 6: the trial state s_trial / vtrial = current (+) x; returns computeScale's sum x (lambda x + b)
  auto apply = [&](double lambda) -> double {
    double sc = 0;
    if (groups & kGsVel) {
      for (int idx = tid; idx < nv; idx += kIiThreads) {
        const int k = order[idx];
        const double* Vk = V + (size_t)k * kIiVtx;
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const double x = Vk[kVx + i];
          sc += x * (lambda * x + Vk[kVb0 + i]);
          vtrial[3 * k + i] = vcur[3 * k + i] + x;
        }
      }
    }
    double scale = block_sum(sc, s_wsum, sum_slot); sum_slot ^= 1;
#pragma unroll
    for (int j = 0; j < 9; j++)
      if ((bmask >> j) & 1) scale += s_xb[j] * (lambda * s_xb[j] + s_rhs0[j]);
    if (tid == 0) {
      IiBorder t = s_cur;
      if (groups & kGsBias) {
#pragma unroll
        for (int i = 0; i < 3; i++) { t.bg[i] += s_xb[i]; t.ba[i] += s_xb[3 + i]; }
      }
      if (groups & kGsGdir) pi_gdir_oplus(t.Rwg, s_xb[6], s_xb[7]);
      if (groups & kGsScale) t.s *= exp(s_xb[8]);
      s_trial = t;
    }
    __syncthreads();
    return scale;
  };

  // computeActiveErrors + activeRobustChi2 at a state (no edge has a robust kernel)
  auto evaluate = [&](const IiBorder& b, const double* vel) -> double {
    double c = 0;
    for (int e = tid; e < ne; e += kIiThreads) {
      const PiGsEdge& E = ed[e];
      double J[kIiJ];
      pi_inertial_gs_edge(E, kf[E.k1].R, kf[E.k1].t, vel + 3 * E.k1, kf[E.k2].R, kf[E.k2].t, vel + 3 * E.k2, b.bg, b.ba, b.Rwg, b.s, 0, J);
      double s = 0;
#pragma unroll
      for (int r = 0; r < 9; r++) {
        double w = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) w += E.info9[9 * r + k] * J[k * kGsLd + kGsColE];
        s += J[r * kGsLd + kGsColE] * w;
      }
      c += s;
    }
    const double chi = block_sum(c, s_wsum, sum_slot) + prior_chi2(b); sum_slot ^= 1;
    return chi;
  };
  auto accept = [&]() {
    if (groups & kGsVel)
      for (int idx = tid; idx < nv; idx += kIiThreads) {
        const int k = order[idx];
#pragma unroll
        for (int i = 0; i < 3; i++) vcur[3 * k + i] = vtrial[3 * k + i];
      }
    if (tid == 0) s_cur = s_trial;
    __syncthreads();
  };
  // the trial velocities of a vertex outside the step are the current ones: an edge reads both ends from one array
  for (int i = tid; i < 3 * nk; i += kIiThreads) vtrial[i] = v0[i];
  __syncthreads();

  double lambda = 0, ni = 2, cur = 0, chi_first = 0;
  int nBad = 0, done = 0, trace_len = 0, failed = 0;
  bool go = true;
  for (int it = 0; it < P.iterations && go; it++) {
    cur = linearise();
    if (it == 0) chi_first = cur;
    const double iniChi = cur;
    if (gn) {
      // G/core/optimization_algorithm_gauss_newton.cpp:50-93: solve, update; a failed solve ends optimize()
      gather();
      const bool ok = solve(0.0);
      if (tid == 0 && trace_len < P.trace_cap) { trace[3 * trace_len] = 0; trace[3 * trace_len + 1] = cur; trace[3 * trace_len + 2] = 1; }
      trace_len++;
      done++;
      if (!ok) { failed = 1; break; }
      apply(0.0);
      accept();
      continue;
    }
    if (it == 0) {
      // computeLambdaInit (G/core/optimization_algorithm_levenberg.cpp:161-174): the user's value, or tau * the largest diagonal entry
      if (P.lambda_init > 0) lambda = P.lambda_init;
      else {
        gather();
        double md = 0;
        if (groups & kGsVel)
          for (int idx = tid; idx < nv; idx += kIiThreads) {
            const double* Vk = V + (size_t)order[idx] * kIiVtx;
            for (int i = 0; i < 3; i++) { const double a = fabs(Vk[i == 0 ? 0 : i == 1 ? 3 : 5]); md = (a < md) ? md : a; }
          }
        s_max[tid] = md;
        __syncthreads();
        md = 0;
        for (int i = 0; i < kIiThreads; i++) { const double a = s_max[i]; md = (a < md) ? md : a; }
#pragma unroll
        for (int j = 0; j < 9; j++)
          if ((bmask >> j) & 1) { const double a = fabs(s_C[10 * j]); md = (a < md) ? md : a; }
        lambda = 1e-5 * md;
      }
      ni = 2; nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    for (;;) {
      gather();
      const bool ok2 = solve(lambda);
      double tempChi = 1.7976931348623157e308, scale = 0;
      if (ok2) {
        scale = apply(lambda);
        tempChi = evaluate(s_trial, vtrial);
      }
      rho = cur - tempChi;
      scale += 1e-3;
      rho /= scale;
      if (rho > 0 && fabs(tempChi) != INFINITY && tempChi == tempChi) {
        double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
        alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;
        const double sf = (1. / 3. < alpha) ? alpha : 1. / 3.;
        lambda *= sf;
        ni = 2;
        cur = tempChi;
        accept();
      } else {
        lambda *= ni; ni *= 2;
      }
      qmax++;
      __syncthreads();
      if (!(rho < 0 && qmax < 10)) break;
    }
    if (tid == 0 && trace_len < P.trace_cap) { trace[3 * trace_len] = lambda; trace[3 * trace_len + 1] = cur; trace[3 * trace_len + 2] = qmax; }
    trace_len++;
    done++;
    if (qmax == 10 || rho == 0) go = false;
    else {
      if ((iniChi - cur) * 1e3 < iniChi) nBad++; else nBad = 0;
      if (nBad >= 3) go = false;
    }
  }
  double chi_final = cur;
  if (gn && !failed && done > 0) chi_final = evaluate(s_cur, vcur);     // Gauss-Newton keeps no chi2 of the estimate it ends on
  __syncthreads();
  for (int i = tid; i < 3 * nk; i += kIiThreads) vout[i] = vcur[i];
  if (tid == 0) {
    out->end = s_cur;
    out->chi2_first = chi_first; out->chi2_final = chi_final;
    out->iters = done; out->solve_failed = failed; out->trace_len = min(trace_len, P.trace_cap);
  }
  solve_word_complete(&out->seq, seq);
}

// the calling thread's work area (common.hpp; the reference calls a static member: no handle)
struct IiBufs {
  orbg::StageBlock stage;
  orbg::DevBuf<double> work;
  void release_buffers() { stage.release(); work.release(); }
};
WorkArea<IiBufs>& ii_work() { static thread_local WorkArea<IiBufs> w; return w; }

// what the checks leave for the solve: the graph as the kernel walks it
struct IiPlan {
  int groups = 0, nv = 0, nb = 0;
  std::vector<int> order, pred, in_edge, out_start, out_edge;
};

// Refusals that need no device.  The predecessor relation must be a forest: every keyframe is k2 of at most one edge (one mPrevKF), and
// following k1 never comes back.  The elimination order is the post-order of a walk from every root in keyframe order, children in
// edge order: a vertex comes after all of its successors.
int ii_check(const inertial_init_problem* p, IiPlan* plan) {
  if (!p || p->struct_size < sizeof(inertial_init_problem)) return ORBG_BAD_ARG;
  if (p->algorithm != INERTIAL_INIT_LM && p->algorithm != INERTIAL_INIT_GN) return ORBG_BAD_ARG;
  if (p->iterations < 0 || p->n_keyframes < 0 || p->n_edges < 0) return ORBG_BAD_ARG;
  if (p->n_keyframes > INERTIAL_INIT_MAX_KEYFRAMES) return ORBG_CAP_EXCEEDED;
  if (p->n_edges < 1 || !p->edges || !p->keyframes) return ORBG_BAD_ARG;                      // no edge
  if (!p->free_velocity && !p->free_bias && !p->free_gdir && !p->free_scale) return ORBG_BAD_ARG;   // no free unknown
  if (p->with_priors && !(p->prior_g >= 0 && p->prior_a >= 0)) return ORBG_BAD_ARG;
  const int nk = p->n_keyframes, ne = p->n_edges;
  plan->groups = (p->free_velocity ? kGsVel : 0) | (p->free_bias ? kGsBias : 0) | (p->free_gdir ? kGsGdir : 0) | (p->free_scale ? kGsScale : 0);
  plan->nb = (p->free_bias ? 6 : 0) + (p->free_gdir ? 2 : 0) + (p->free_scale ? 1 : 0);
  plan->pred.assign(nk, -1); plan->in_edge.assign(nk, -1); plan->out_start.assign(nk + 1, 0); plan->out_edge.assign(ne, 0);
  for (int e = 0; e < ne; e++) {
    const int k1 = p->edges[e].k1, k2 = p->edges[e].k2;
    if (k1 < 0 || k1 >= nk || k2 < 0 || k2 >= nk) return ORBG_BAD_ARG;
    if (plan->in_edge[k2] >= 0) return ORBG_BAD_ARG;                                          // two mPrevKF
    plan->in_edge[k2] = e; plan->pred[k2] = k1;
    plan->out_start[k1 + 1]++;
  }
  for (int k = 0; k < nk; k++) plan->out_start[k + 1] += plan->out_start[k];
  {
    std::vector<int> fill(plan->out_start.begin(), plan->out_start.end() - 1);
    for (int e = 0; e < ne; e++) plan->out_edge[fill[p->edges[e].k1]++] = e;
  }
  int in_system = 0;
  for (int k = 0; k < nk; k++) in_system += plan->in_edge[k] >= 0 || plan->out_start[k + 1] > plan->out_start[k];
  plan->order.clear(); plan->order.reserve(in_system);
  std::vector<int> stack, next(nk, 0);
  for (int root = 0; root < nk; root++) {
    if (plan->in_edge[root] >= 0 || plan->out_start[root + 1] == plan->out_start[root]) continue;
    stack.push_back(root);
    while (!stack.empty()) {
      const int k = stack.back();
      const int o = plan->out_start[k] + next[k];
      if (o < plan->out_start[k + 1]) { next[k]++; stack.push_back(p->edges[plan->out_edge[o]].k2); }
      else { plan->order.push_back(k); stack.pop_back(); }
    }
  }
  if ((int)plan->order.size() != in_system) return ORBG_BAD_ARG;                               // a cycle: no root reaches it
  plan->nv = in_system;
  return ORBG_OK;
}

void ii_fill_edge(const inertial_init_edge& s, PiGsEdge* d) {
  const pose_inertial_preint& I = s.preint;
  d->k1 = s.k1; d->k2 = s.k2;
  d->dT = I.dT;
  for (int i = 0; i < 9; i++) { d->dR[i] = I.dR[i]; d->JRg[i] = I.JRg[i]; d->JVg[i] = I.JVg[i]; d->JVa[i] = I.JVa[i]; d->JPg[i] = I.JPg[i]; d->JPa[i] = I.JPa[i]; }
  for (int i = 0; i < 3; i++) { d->dV[i] = I.dV[i]; d->dP[i] = I.dP[i]; d->lbg[i] = I.bg[i]; d->lba[i] = I.ba[i]; }
  memcpy(d->info9, s.info9, sizeof(d->info9));
}
void ii_fill_border(const inertial_init_problem* p, IiBorder* b) {
  for (int i = 0; i < 3; i++) { b->bg[i] = p->bg[i]; b->ba[i] = p->ba[i]; }
  memcpy(b->Rwg, p->Rwg, sizeof(b->Rwg));
  b->s = p->scale;
}

}  // namespace

// the calling thread's inertial_init_solve calls on `device` use the caller's stream from now on (NULL: the library's M stream again)
extern "C" int inertial_init_set_stream(int device, void* hip_stream) {
  WorkArea<IiBufs>& sc = ii_work();
  int rc = sc.open(device, "po");
  if (rc) return rc;
  return orbg::swap_stream(&sc.stream, &sc.ext_stream, hip_stream, "po");
}

extern "C" int inertial_init_host_linearize(const inertial_init_problem* p, double* J) {
  IiPlan plan;
  const int rc = ii_check(p, &plan);
  if (rc) return rc;
  if (!J) return ORBG_BAD_ARG;
  IiBorder b;
  ii_fill_border(p, &b);
  for (int e = 0; e < p->n_edges; e++) {
    PiGsEdge E;
    ii_fill_edge(p->edges[e], &E);
    double R[2][9], t[2][3], v[2][3];
    for (int q = 0; q < 2; q++) {
      const pose_inertial_state& s = p->keyframes[q ? E.k2 : E.k1];
      for (int i = 0; i < 9; i++) R[q][i] = s.Rwb[i];
      for (int i = 0; i < 3; i++) { t[q][i] = s.twb[i]; v[q][i] = s.vwb[i]; }
    }
    pi_inertial_gs_edge(E, R[0], t[0], v[0], R[1], t[1], v[1], b.bg, b.ba, b.Rwg, b.s, kGsAll, J + (size_t)e * kIiJ);
  }
  return ORBG_OK;
}

extern "C" int inertial_init_solve(const inertial_init_problem* p, inertial_init_result* r) {
  if (!r || r->struct_size < sizeof(inertial_init_result)) return ORBG_BAD_ARG;
  IiPlan plan;
  const int crc = ii_check(p, &plan);
  if (crc) return crc;
  if (!r->vwb || r->trace_cap < 0 || (r->trace_cap > 0 && !r->trace)) return ORBG_BAD_ARG;
  WorkArea<IiBufs>& sc = ii_work();
  int rc = sc.open(p->device, "po");
  if (rc) return rc;
  const int nk = p->n_keyframes, ne = p->n_edges, nv = plan.nv, tcap = r->trace_cap;
  // one staging block: the result record, the velocities and the trace are written in place (mapped); the parameters, the poses, the
  // edges and the graph, which every iteration re-reads, get the block's one copy to the device
  orbg::StageBlock& S = sc.stage;
  const size_t payload = sizeof(IiOut) + sizeof(IiParams) + (size_t)nk * (sizeof(IiKf) + 6 * sizeof(double) + 3 * sizeof(int) + sizeof(int)) + sizeof(int) +
                         (size_t)ne * (sizeof(PiGsEdge) + sizeof(int)) + (size_t)tcap * 3 * sizeof(double);
  if ((rc = S.begin(orbg::StageLayout::bound(12, payload)))) return rc;
  const auto s_out = S.room<IiOut>(1);
  const auto s_vout = S.room<double>(3 * (size_t)nk);
  const auto s_trace = S.room<double>(3 * (size_t)tcap);
  const auto s_prm = S.room<IiParams>(1, true);
  const auto s_kf = S.room<IiKf>(nk, true);
  const auto s_v0 = S.room<double>(3 * (size_t)nk, true);
  const auto s_ed = S.room<PiGsEdge>(ne, true);
  const int* d_order = S.add(plan.order.data(), (size_t)nv, true);
  const int* d_pred = S.add(plan.pred.data(), (size_t)nk, true);
  const int* d_in = S.add(plan.in_edge.data(), (size_t)nk, true);
  const int* d_os = S.add(plan.out_start.data(), (size_t)nk + 1, true);
  const int* d_oe = S.add(plan.out_edge.data(), (size_t)ne, true);
  {
    IiParams* P = S.host(s_prm);
    memset(P, 0, sizeof(IiParams));
    P->nk = nk; P->ne = ne; P->nv = nv; P->algorithm = p->algorithm; P->iterations = p->iterations; P->groups = plan.groups;
    P->priors = (p->with_priors && p->free_bias) ? 1 : 0;          // an edge whose vertices are all fixed is not active (sparse_optimizer.cpp:234)
    P->trace_cap = tcap;
    P->lambda_init = p->lambda_init; P->prior_g = p->prior_g; P->prior_a = p->prior_a;
    ii_fill_border(p, &P->start);
    IiKf* K = S.host(s_kf);
    double* v0 = S.host(s_v0);
    for (int k = 0; k < nk; k++) {
      const pose_inertial_state& s = p->keyframes[k];
      for (int i = 0; i < 9; i++) K[k].R[i] = s.Rwb[i];
      for (int i = 0; i < 3; i++) { K[k].t[i] = s.twb[i]; v0[3 * k + i] = s.vwb[i]; }
    }
    PiGsEdge* E = S.host(s_ed);
    for (int e = 0; e < ne; e++) ii_fill_edge(p->edges[e], &E[e]);
  }
  if ((rc = S.commit(sc.stream))) return rc;
  const bool lds = nk <= kIiTile;
  const size_t wJ = (size_t)ne * kIiJ, wH = (size_t)ne * kIiH, wV = lds ? 0 : (size_t)nk * kIiVtx, wv = 3 * (size_t)nk;
  if ((rc = sc.work.reserve(wJ + wH + wV + 2 * wv))) return rc;
  double* dJ = sc.work.p; double* dH = dJ + wJ; double* dV = dH + wH; double* dvc = dV + wV; double* dvt = dvc + wv;
  static thread_local orbg::SolveWord done_word;
  IiOut* ho = S.host(s_out);
  const unsigned ii_seq = done_word.arm(&ho->seq);
  if (lds)
    hipLaunchKernelGGL(inertial_init_kernel<true>, dim3(1), dim3(kIiThreads), 0, sc.stream, (const IiParams*)S.device(s_prm), (const IiKf*)S.device(s_kf),
                       (const PiGsEdge*)S.device(s_ed), (const double*)S.device(s_v0), d_order, d_pred, d_in, d_os, d_oe, dJ, dH, dV, dvc, dvt,
                       S.mapped(s_out), S.mapped(s_vout), S.mapped(s_trace), ii_seq);
  else
    hipLaunchKernelGGL(inertial_init_kernel<false>, dim3(1), dim3(kIiThreads), 0, sc.stream, (const IiParams*)S.device(s_prm), (const IiKf*)S.device(s_kf),
                       (const PiGsEdge*)S.device(s_ed), (const double*)S.device(s_v0), d_order, d_pred, d_in, d_os, d_oe, dJ, dH, dV, dvc, dvt,
                       S.mapped(s_out), S.mapped(s_vout), S.mapped(s_trace), ii_seq);
  ORBG_HIP(hipGetLastError());
  if ((rc = done_word.wait(sc.stream))) return rc;
  S.get(s_vout, r->vwb);
  memcpy(r->bg, ho->end.bg, sizeof(r->bg)); memcpy(r->ba, ho->end.ba, sizeof(r->ba)); memcpy(r->Rwg, ho->end.Rwg, sizeof(r->Rwg));
  r->scale = ho->end.s;
  r->iters = ho->iters; r->solve_failed = ho->solve_failed;
  r->n_unknowns = ((plan.groups & kGsVel) ? 3 * nv : 0) + plan.nb;
  r->chi2_first = ho->chi2_first; r->chi2_final = ho->chi2_final;
  r->trace_len = ho->trace_len;
  if (r->trace_len > 0) memcpy(r->trace, S.host(s_trace), (size_t)r->trace_len * 3 * sizeof(double));
  return ORBG_OK;
}
