// liborbgpu -- the local bundle adjustment of an inertial agent for gfx950 (MI355X).  Replaces the numerical core of
// Optimizer::LocalInertialBA (S/Optimizer.cc:4556-5226, called from LocalMapping::Run once the IMU is initialised) behind
// inertial_ba_solve() of include/orbgpu.h: ONE optimize(10, or 4 when bLarge) of g2o's Levenberg-Marquardt with the user's lambda over
// a window of keyframes chained by EdgeInertial / EdgeGyroRW / EdgeAccRW, their map points (marginalised) and the fixed keyframes that
// observe them.
//
// The vertices and the inertial edges are the per-frame optimiser's (pose_inertial_edges.hpp), the LM decisions and the LDL^T solvers
// the bundle adjustments' (lm_step.hpp, lm_driver.hpp, lm_record.hpp, ldlt_solver.hpp), the landmark-Schur arithmetic full_ba.hip's (landmark_schur.hpp).  What is new:
// the visual edges in the ImuCamPose parametrisation (update on the body, right-multiplied rotation), keyframe blocks of 15 (6 without
// an IMU) at the offsets of a table, and the inertial blocks in the reduced system.
//   structure, once per call, on the host (a window holds at most 32 free keyframes): the run of edges of every point, the edges of
//     every free keyframe in ascending order, the non-empty keyframe pairs with their (edge of i, edge of j) items in the order of
//     keyframe i's list, and per pair the inertial edges that add to its block, in edge order
//   per LM iteration:
//     k_iba_edges   blocks [0, nbe): thread/visual edge  error, chi2, rho, Jacobians -> Hpl | Hll | bl | Hpp | bp
//                   blocks [nbe, nbe + nIE): workgroup/inertial edge  the stacked 15 x 30 Jacobian (EdgeInertial's rows on thread 0,
//                   the random walks' on thread 64), then across the workgroup W J, rho, J^T (rho W) J | b
//     k_schur_points thread/point Hll, bl in edge order;  k_iba_poses  workgroup/free keyframe  Hpp, bp (fixed tree)
//     k_iba_finish  the robust chi2 of the evaluation -> the record the host reads
//   per trial:
//     k_schur_dinv  thread/point (Hll + lambda I)^-1 and its product with bl
//     one fill of the dense reduced system, then k_iba_schur: workgroup per NON-EMPTY pair, the visual items in fixed order, then the
//       pair's inertial blocks in edge order, one thread per entry
//     LDL^T by size (LdltSolver::plan)
//     k_iba_update  thread/vertex  back-substitution, ImuCamPose::Update, trial state (a full copy), computeScale terms
//     k_iba_edges without the block outputs (errors of the trial state, visual and inertial) + k_iba_finish   robust chi2, scale
// Launches and waits per trial are those of ba_solve.  Every sum has a fixed order, no floating-point atomic: two calls on the same
// input return the same bits.  All of it in double.

#include <time.h>
#include <unistd.h>

#include <atomic>

#include "common.hpp"
#include "wave.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <type_traits>
#include <vector>

#include "lm_driver.hpp"
#include "lm_record.hpp"

using namespace orbg;
using namespace orbg_lm;

namespace {

#include "ldlt_mfma.hpp"
#include "ldlt_xcd.hpp"
#include "ldlt_wide.hpp"
#include "ldlt_solver.hpp"
#include "pose_inertial_edges.hpp"
#include "landmark_schur.hpp"

constexpr int kIbaMaxFree = INERTIAL_BA_MAX_FREE_KEYFRAMES;
constexpr int kIbaEB = 54;               // per visual edge: Hpl (6 x 3, 18) | Hll upper (6) | bl (3) | Hpp upper (21) | bp (6)
constexpr int kIbaIW = 31;               // row stride of an inertial edge's block: [keyframe 1's 15 | keyframe 2's 15 | b]
constexpr int kIbaIB = 30 * kIbaIW;      // J^T (rho W) J (30 x 30) with -J^T (rho W) e in the last column
constexpr int kIbaThreads = 256;
static_assert(kIbaEB == kSchurHead + 21 + 6, "an edge's block is what landmark_schur.hpp reads (Hpl | Hll | bl), then the edge's Hpp | bp");
static_assert(kIbaThreads == kSchurThreads, "k_iba_edges reduces with block_sum_256, and the shared loops advance by this workgroup size");

struct IbaCam { double fx, fy, cx, cy, bf, Rcb[9], tcb[3], tbc[3]; };
struct IbaInertial { int k1, k2, robust, pad; };          // EdgeInertial + EdgeGyroRW + EdgeAccRW between keyframes k1 (the earlier) and k2
struct IbaPairInertial { int e, ro, co; };                // block (ro.., co..) of inertial edge e adds to the pair's block

// ---------------------------------------------------------------------------------------------- the visual edges (host and device)

// EdgeMono / EdgeStereo::computeError (I/G2oTypes.h: obs - VPose->estimate().Project / ProjectStereo(VPoint->estimate()))
struct IbaVis { double e[3], c2, Xc[3]; };
PI_HD __forceinline__ void iba_visual_error(const double* cam, const IbaCam& C, const double* X, float u, float v, float ur, double om, IbaVis* o) {
#pragma unroll
  for (int i = 0; i < 3; i++) o->Xc[i] = cam[3 * i] * X[0] + cam[3 * i + 1] * X[1] + cam[3 * i + 2] * X[2] + cam[9 + i];
  const double pu = C.fx * o->Xc[0] / o->Xc[2] + C.cx, pv = C.fy * o->Xc[1] / o->Xc[2] + C.cy;
  o->e[0] = (double)u - pu;
  o->e[1] = (double)v - pv;
  o->e[2] = ur < 0 ? 0.0 : (double)ur - (pu - C.bf * (1.0 / o->Xc[2]));
  o->c2 = o->e[0] * (om * o->e[0]) + o->e[1] * (om * o->e[1]) + o->e[2] * (om * o->e[2]);
}
// linearizeOplus (S/G2oTypes.cc:349-373, 397-427): Jl = -proj_jac Rcw (3 x 3), Jp = proj_jac Rcb SE3deriv(Xb) (3 x 6); the third rows
// are the stereo edge's (row 0 plus bf / z^2 in column 2), zero for a monocular edge
PI_HD __forceinline__ void iba_visual_jacobians(const IbaVis& o, const double* cam, const IbaCam& C, bool mono, double* Jl, double* Jp) {
  const double x = o.Xc[0], y = o.Xc[1], z = o.Xc[2], iz2 = 1.0 / (z * z);
  double pj[9] = {C.fx / z, 0.0, -C.fx * x * iz2, 0.0, C.fy / z, -C.fy * y * iz2, 0.0, 0.0, 0.0};
  if (!mono) { pj[6] = pj[0]; pj[8] = pj[2] + C.bf * iz2; }
  double M[9], Xb[3];
  m3_mul(pj, cam, M);
#pragma unroll
  for (int i = 0; i < 9; i++) Jl[i] = -M[i];
  m3_mul(pj, C.Rcb, M);
  m3_tvec(C.Rcb, o.Xc, Xb);
#pragma unroll
  for (int i = 0; i < 3; i++) Xb[i] += C.tbc[i];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    Jp[6 * k] = -M[3 * k + 1] * Xb[2] + M[3 * k + 2] * Xb[1];
    Jp[6 * k + 1] = M[3 * k] * Xb[2] - M[3 * k + 2] * Xb[0];
    Jp[6 * k + 2] = -M[3 * k] * Xb[1] + M[3 * k + 1] * Xb[0];
    Jp[6 * k + 3] = M[3 * k]; Jp[6 * k + 4] = M[3 * k + 1]; Jp[6 * k + 5] = M[3 * k + 2];
  }
}
// the edge's blocks of the normal equations with the weight w = rho1 * omega: out[kIbaEB]
PI_HD __forceinline__ void iba_visual_blocks(const IbaVis& o, const double* Jl, const double* Jp, double w, double* out) {
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * a + c] = Jp[a] * (w * Jl[c]) + Jp[6 + a] * (w * Jl[3 + c]) + Jp[12 + a] * (w * Jl[6 + c]);
  int q = 18;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int c = a; c < 3; c++) out[q++] = Jl[a] * (w * Jl[c]) + Jl[3 + a] * (w * Jl[3 + c]) + Jl[6 + a] * (w * Jl[6 + c]);
#pragma unroll
  for (int a = 0; a < 3; a++) out[q++] = -(Jl[a] * (w * o.e[0]) + Jl[3 + a] * (w * o.e[1]) + Jl[6 + a] * (w * o.e[2]));
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int c = a; c < 6; c++) out[q++] = Jp[a] * (w * Jp[c]) + Jp[6 + a] * (w * Jp[6 + c]) + Jp[12 + a] * (w * Jp[12 + c]);
#pragma unroll
  for (int a = 0; a < 6; a++) out[q++] = -(Jp[a] * (w * o.e[0]) + Jp[6 + a] * (w * o.e[1]) + Jp[12 + a] * (w * o.e[2]));
}
// EdgeGyroRW, EdgeAccRW (I/G2oTypes.h:632-701) between s1 and s2: rows 9..14 of the stacked Jacobian, columns as pi_inertial_edge's
PI_HD inline void iba_walk_edges(const PiState& s1, const PiState& s2, double* J) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    J[(9 + i) * kPiLd + 30] = s2.bg[i] - s1.bg[i];
    J[(12 + i) * kPiLd + 30] = s2.ba[i] - s1.ba[i];
    J[(9 + i) * kPiLd + 9 + i] = -1.0; J[(9 + i) * kPiLd + 24 + i] = 1.0;
    J[(12 + i) * kPiLd + 12 + i] = -1.0; J[(12 + i) * kPiLd + 27 + i] = 1.0;
  }
}
// the information entry (r, k) of the stacked rows: EdgeInertial's 9 x 9, then the two 3 x 3
PI_HD __forceinline__ void iba_row_block(int r, int* r0, int* bw) {
  if (r < 9) { *r0 = 0; *bw = 9; }
  else if (r < 12) { *r0 = 9; *bw = 3; }
  else { *r0 = 12; *bw = 3; }
}
PI_HD __forceinline__ double iba_info(const PiParams& P, int r, int k) {
  return r < 9 ? P.info9[9 * r + k] : r < 12 ? P.infoG[3 * (r - 9) + k] : P.infoA[3 * (r - 12) + k];
}

// ---------------------------------------------------------------------------------------------- kernels

// One inertial edge, the whole workgroup: thread 0 EdgeInertial's rows, thread 64 the random walks' (the transcendental part), then
// W J, the three chi2 and -- with IB -- J^T (rho W) J | -J^T (rho W) e, one entry per thread and pass.  Returns in thread 0 the sum
// of the three robustified chi2 (only EdgeInertial may have a kernel: delta sqrt(16.92), S/Optimizer.cc:4826-4837).
__device__ __forceinline__ void iba_inertial_block(const IbaInertial ie, const PiParams& P, const PiState* __restrict__ kfs, double* __restrict__ IB,
                                                   double* __restrict__ chi_out) {
  __shared__ double s_J[15 * kPiLd], s_WJ[15 * kPiLd];
  __shared__ double s_rho1;
  const int tid = threadIdx.x;
  for (int i = tid; i < 15 * kPiLd; i += kIbaThreads) s_J[i] = 0;
  __syncthreads();
  if (tid == 0) pi_inertial_edge(P, kfs[ie.k1], kfs[ie.k2], true, 15, 30, s_J);
  if (tid == 64) iba_walk_edges(kfs[ie.k1], kfs[ie.k2], s_J);
  __syncthreads();
  for (int id = tid; id < 15 * kIbaIW; id += kIbaThreads) {
    const int r = id / kIbaIW, c = id % kIbaIW;
    int r0, bw;
    iba_row_block(r, &r0, &bw);
    double s = 0;
    for (int k = 0; k < bw; k++) s += iba_info(P, r, k) * s_J[(r0 + k) * kPiLd + c];
    s_WJ[r * kPiLd + c] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double cI = 0, cG = 0, cA = 0;
    for (int r = 0; r < 9; r++) cI += s_J[r * kPiLd + 30] * s_WJ[r * kPiLd + 30];
    for (int r = 9; r < 12; r++) cG += s_J[r * kPiLd + 30] * s_WJ[r * kPiLd + 30];
    for (int r = 12; r < 15; r++) cA += s_J[r * kPiLd + 30] * s_WJ[r * kPiLd + 30];
    double rho0 = cI, rho1 = 1.0;
    if (ie.robust) pi_huber(cI, sqrt(16.92), &rho0, &rho1);
    s_rho1 = rho1;
    *chi_out = (rho0 + cG) + cA;
  }
  if (!IB) return;
  __syncthreads();
  const double rho1 = s_rho1;
  for (int id = tid; id < kIbaIB; id += kIbaThreads) {
    const int a = id / kIbaIW, c = id % kIbaIW;
    double si = 0, sw = 0;
    for (int r = 0; r < 9; r++) si += s_J[r * kPiLd + a] * s_WJ[r * kPiLd + c];
    for (int r = 9; r < 15; r++) sw += s_J[r * kPiLd + a] * s_WJ[r * kPiLd + c];
    const double s = rho1 * si + sw;
    IB[id] = c == 30 ? -s : s;
  }
}

// computeActiveErrors (+ with EB / IEB the edges' part of buildSystem) of state (kfs, points).  Blocks [0, nbe): one visual edge per
// thread; blocks [nbe, nbe + nIE): one inertial edge per workgroup.  partial[block] = the block's robustified chi2.
__global__ __launch_bounds__(kIbaThreads) void k_iba_edges(int NE, int nbe, const lba_edge* __restrict__ edges, const PiState* __restrict__ kfs,
                                                           const double* __restrict__ points, IbaCam C, double dM, double dS,
                                                           const IbaInertial* __restrict__ ies, const PiParams* __restrict__ ieP,
                                                           double* __restrict__ chi2, double* __restrict__ partial, double* __restrict__ EB,
                                                           double* __restrict__ IEB) {
  if ((int)blockIdx.x >= nbe) {
    const int e = blockIdx.x - nbe;
    iba_inertial_block(ies[e], ieP[e], kfs, IEB ? IEB + (size_t)e * kIbaIB : nullptr, partial + blockIdx.x);
    return;
  }
  __shared__ double red[4];
  const int k = blockIdx.x * kIbaThreads + threadIdx.x;
  double rho0 = 0;
  if (k < NE) {
    const lba_edge e = edges[k];
    double cam[12];
    pi_camera_pose(kfs[e.pose], C.Rcb, C.tcb, cam);
    const bool mono = e.ur < 0;
    const double om = (double)e.inv_sigma2;
    IbaVis o;
    iba_visual_error(cam, C, points + 3 * (size_t)e.point, e.u, e.v, e.ur, om, &o);
    chi2[k] = o.c2;
    double rho1;
    pi_huber(o.c2, mono ? dM : dS, &rho0, &rho1);
    if (EB) {
      double Jl[9], Jp[18];
      iba_visual_jacobians(o, cam, C, mono, Jl, Jp);
      iba_visual_blocks(o, Jl, Jp, rho1 * om, EB + (size_t)k * kIbaEB);
    }
  }
  const double s = block_sum_256(rho0, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Hpp (21 upper entries), bp of the visual edges of one free keyframe: thread t takes edges t, t + 256, ... of its list in order
__global__ __launch_bounds__(256) void k_iba_poses(const int* __restrict__ row_start, const int* __restrict__ row_edges,
                                                   const double* __restrict__ EB, double* __restrict__ Hpp, double* __restrict__ bp) {
  const int p = blockIdx.x;
  const int b = row_start[p], e_end = row_start[p + 1];
  double acc[27];
#pragma unroll
  for (int i = 0; i < 27; i++) acc[i] = 0;
  for (int q = b + threadIdx.x; q < e_end; q += 256) {
    const double* eb = EB + (size_t)row_edges[q] * kIbaEB + kSchurHead;
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] += eb[i];
  }
  schur_pose_tail(acc, p, Hpp, bp);
}

// The block of the reduced system of one NON-EMPTY pair of free keyframes (i1 <= i2, widths d1, d2 of 6 or 15, columns from the
// table): [i1 == i2](Hpp + lambda I) - sum_l Hpl_i1l Dinv_l Hpl_i2l^T in its upper-left 6 x 6, over the pair's items in fixed order,
// plus the blocks of the pair's inertial edges in edge order.  Diagonal pairs also the right-hand side and bk, the keyframe's b
// before the landmarks are eliminated (computeScale reads it).  Blocks of absent pairs keep the zeros of the fill.
__global__ __launch_bounds__(256) void k_iba_schur(int n, const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                   const int* __restrict__ col_off, const int* __restrict__ col_dim,
                                                   const int* __restrict__ item_start, const SchurItem* __restrict__ items,
                                                   const int* __restrict__ pie_start, const IbaPairInertial* __restrict__ pies,
                                                   const lba_edge* __restrict__ edges, const double* __restrict__ EB, const double* __restrict__ IEB,
                                                   const double* __restrict__ Dinv, const double* __restrict__ Db,
                                                   const double* __restrict__ Hpp, const double* __restrict__ bp, double lambda,
                                                   double* __restrict__ S, double* __restrict__ bs, double* __restrict__ bk, double* __restrict__ St) {
  __shared__ double wpart[4][42];
  const int p = blockIdx.x;
  const int i1 = pair_i[p], i2 = pair_j[p];
  const bool diag = i1 == i2;
  const int b = item_start[p], e = item_start[p + 1];
  schur_pair_items<kIbaEB>(diag, b, e, items, edges, EB, Dinv, Db, wpart);
  const int tid = threadIdx.x;
  const int d1 = col_dim[i1], d2 = col_dim[i2], c1 = col_off[i1], c2 = col_off[i2];
  const int pb = pie_start[p], pe = pie_start[p + 1];
  // every entry of the system and its mirror image are written by ONE thread, with one value: on a diagonal pair the thread of
  // (a, c), a <= c, alone
  if (tid < 225) {
    const int a = tid / 15, c = tid % 15;
    if (a >= d1 || c >= d2 || (diag && a > c)) return;
    double v = 0;
    if (a < 6 && c < 6) {
      const int w = 6 * a + c;
      v = -(((wpart[0][w] + wpart[1][w]) + wpart[2][w]) + wpart[3][w]);
      if (diag) v += Hpp[21 * (size_t)i1 + a * 6 - a * (a - 1) / 2 + (c - a)];
    }
    if (diag && a == c) v += lambda;
    for (int q = pb; q < pe; q++) { const IbaPairInertial pi = pies[q]; v += IEB[(size_t)pi.e * kIbaIB + (pi.ro + a) * kIbaIW + pi.co + c]; }
    const int r = c1 + a, cc = c2 + c;
    schur_store_entry(r, cc, n, v, S, St);
  } else if (diag && tid < 240) {
    const int a = tid - 225;
    if (a >= d1) return;
    double v = 0, s = 0;
    if (a < 6) {
      const int w = 36 + a;
      s = ((wpart[0][w] + wpart[1][w]) + wpart[2][w]) + wpart[3][w];
      v = bp[6 * (size_t)i1 + a];
    }
    for (int q = pb; q < pe; q++) { const IbaPairInertial pi = pies[q]; v += IEB[(size_t)pi.e * kIbaIB + (pi.ro + a) * kIbaIW + 30]; }
    bk[c1 + a] = v;
    v -= s;
    bs[c1 + a] = v;
    if (St) ldltm::image_put_rhs(St, n, c1 + a, v);
  }
}

// trial state = oplus(current, x), a full copy; per vertex its term of computeScale: sum_j x_j (lambda x_j + b_j)
__global__ __launch_bounds__(256) void k_iba_update(int NK, int NX, const int* __restrict__ kf_col, const int* __restrict__ col_off,
                                                    const int* __restrict__ col_dim, const PiState* __restrict__ kfs,
                                                    const double* __restrict__ points, const double* __restrict__ x,
                                                    const int* __restrict__ pt_start, const int* __restrict__ pt_end,
                                                    const lba_edge* __restrict__ edges, const double* __restrict__ EB,
                                                    const double* __restrict__ Dinv, const double* __restrict__ bl,
                                                    const double* __restrict__ bk, double lambda, const int* __restrict__ ok_flag,
                                                    PiState* __restrict__ kfs_out, double* __restrict__ points_out, double* __restrict__ scale_v) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= NK + NX) return;
  const bool ok = *ok_flag != 0;                   // a failed solve leaves no step: the trial state is the current one
  if (v < NK) {
    const int c = kf_col[v];
    double sc = 0;
    PiState T = kfs[v];
    if (c >= 0 && ok) {
      const int o = col_off[c], d = col_dim[c];
      double u[15];
#pragma unroll
      for (int a = 0; a < 15; a++) {
        u[a] = a < d ? x[o + a] : 0.0;
        if (a < d) sc += u[a] * (lambda * u[a] + bk[o + a]);
      }
      pi_oplus(&T, u);
    }
    kfs_out[v] = T;
    scale_v[v] = sc;
    return;
  }
  schur_update_point<kIbaEB>(v - NK, ok, kf_col, [col_off](int c) { return col_off[c]; }, points, x, pt_start, pt_end, edges, EB, Dinv, bl, lambda,
                             points_out, scale_v + v);
}

// one workgroup: the sums of the partials and of the scale terms in index order, the solver's flag -> the record
__global__ __launch_bounds__(256) void k_iba_finish(int n_partial, const double* __restrict__ partial, int n_scale, const double* __restrict__ scale_v,
                                                    const int* __restrict__ ok_flag, LmRec* __restrict__ rec) {
  lm_finish_record<false>(n_partial, partial, n_scale, scale_v, 0.0, ok_flag, rec);   // (the user's lambda is always positive: nobody reads maxdiag)
}

// ImuCamPose::isDepthPositive (S/G2oTypes.cc:187-190) of every visual edge
__global__ __launch_bounds__(256) void k_iba_depth(int NE, const lba_edge* __restrict__ edges, const PiState* __restrict__ kfs,
                                                   const double* __restrict__ points, IbaCam C, uint8_t* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= NE) return;
  const lba_edge e = edges[k];
  double cam[12];
  pi_camera_pose(kfs[e.pose], C.Rcb, C.tcb, cam);
  const double* X = points + 3 * (size_t)e.point;
  out[k] = cam[6] * X[0] + cam[7] * X[1] + cam[8] * X[2] + cam[11] > 0.0 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- host

void iba_widen_state(const pose_inertial_state& s, PiState* d) {
  for (int i = 0; i < 9; i++) d->R[i] = s.Rwb[i];
  for (int i = 0; i < 3; i++) { d->t[i] = s.twb[i]; d->v[i] = s.vwb[i]; d->bg[i] = s.bg[i]; d->ba[i] = s.ba[i]; }
}

void iba_fill_cam(const inertial_ba_problem* p, IbaCam* C) {
  C->fx = p->fx; C->fy = p->fy; C->cx = p->cx; C->cy = p->cy; C->bf = p->bf;
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) C->Rcb[3 * i + j] = p->Tcb[4 * i + j]; C->tcb[i] = p->Tcb[4 * i + 3]; }
  double t[3];
  m3_tvec(C->Rcb, C->tcb, t);                      // tbc = -Rbc tcb
  for (int i = 0; i < 3; i++) C->tbc[i] = -t[i];
}

// the inertial edge of keyframe k2 as the kernel reads it: every float widened; the information of the window's last edge is
// multiplied by 1e-2 (S/Optimizer.cc:4834-4835)
void iba_fill_inertial(const inertial_ba_keyframe& kf, PiParams* P) {
  memset(P, 0, sizeof(PiParams));
  const pose_inertial_preint& I = kf.preint;
  P->dT = I.dT;
  for (int i = 0; i < 9; i++) { P->dR[i] = I.dR[i]; P->JRg[i] = I.JRg[i]; P->JVg[i] = I.JVg[i]; P->JVa[i] = I.JVa[i]; P->JPg[i] = I.JPg[i]; P->JPa[i] = I.JPa[i]; }
  for (int i = 0; i < 3; i++) { P->dV[i] = I.dV[i]; P->dP[i] = I.dP[i]; P->lbg[i] = I.bg[i]; P->lba[i] = I.ba[i]; }
  for (int i = 0; i < 81; i++) P->info9[i] = kf.last_in_window ? kf.info9[i] * 1e-2 : kf.info9[i];
  memcpy(P->infoG, kf.infoG, sizeof(P->infoG)); memcpy(P->infoA, kf.infoA, sizeof(P->infoA));
}

inline bool iba_edge_is_right(float ur) { return ur == LBA_UR_RIGHT_CAMERA; }

// What can be refused is refused here, before a device is selected or anything is launched.
int iba_validate(const inertial_ba_problem* p, const inertial_ba_result* r, int* n_free, int* n_unknowns) {
  if (!p || !r) return ORBG_BAD_ARG;
  if (p->struct_size < sizeof(inertial_ba_problem) || r->struct_size < sizeof(inertial_ba_result)) return ORBG_BAD_ARG;
  if (p->n_keyframes <= 0 || p->n_points < 0 || p->n_edges < 0) return ORBG_BAD_ARG;
  if (!p->keyframes || !r->states) return ORBG_BAD_ARG;
  if (p->n_points > 0 && (!p->points || !p->close || !r->points)) return ORBG_BAD_ARG;
  if (p->n_edges > 0 && (!p->edges || p->n_points == 0)) return ORBG_BAD_ARG;
  if (r->trace && r->trace_cap < 0) return ORBG_BAD_ARG;
  if (p->n_edges > INERTIAL_BA_MAX_EDGES) return ORBG_CAP_EXCEEDED;
  int nF = 0, n = 0;
  for (int i = 0; i < p->n_keyframes; i++) {
    const inertial_ba_keyframe& kf = p->keyframes[i];
    if (!kf.fixed) { nF++; n += kf.imu ? 15 : 6; }
    if (kf.last_in_window && !kf.link) return ORBG_BAD_ARG;
    if (!kf.link) continue;
    // EdgeInertial ends in a free keyframe of the window; both ends carry velocity and biases (bImu)
    if (kf.fixed || !kf.imu || kf.prev < 0 || kf.prev >= p->n_keyframes || kf.prev == i || !p->keyframes[kf.prev].imu) return ORBG_BAD_ARG;
  }
  if (nF == 0) return ORBG_BAD_ARG;
  if (nF > kIbaMaxFree) return ORBG_CAP_EXCEEDED;
  *n_free = nF; *n_unknowns = n;
  // (EdgeMono(1), the right camera of a rig: not part of this entry point)
  return schur_check_edges(p->edges, p->n_edges, p->n_keyframes, p->n_points, iba_edge_is_right);
}

}  // namespace

struct inertial_ba_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  bool ext_stream = false;
  LdltSolver ldlt;
  DevBuf<lba_edge> d_edges;
  DevBuf<PiState> d_kfs[2];
  DevBuf<double> d_points[2];
  DevBuf<int> d_ints, d_ok;               // the structure's integer tables, one upload
  DevBuf<SchurItem> d_items;
  DevBuf<IbaPairInertial> d_pies;
  DevBuf<IbaInertial> d_ies;
  DevBuf<PiParams> d_ieP;
  DevBuf<double> d_chi2, d_partial, d_EB, d_IEB, d_Hll, d_bl, d_Hpp, d_bp, d_Dinv, d_Db, d_bs, d_bk, d_x, d_scale_v;
  DevBuf<uint8_t> d_depth;
  DevBuf<LmRec> d_rec;
  PinnedBuf<LmRec> rec;
  std::vector<PiState> s_kfs;
  std::vector<double> s_points;
  std::vector<int> s_ints;
  std::vector<SchurItem> s_items;
  std::vector<IbaPairInertial> s_pies;
  std::vector<IbaInertial> s_ies;
  std::vector<PiParams> s_ieP;
  PhaseTimer<5> timer;                 // inertial_ba_set_profiling
};

namespace {

enum { kPhStructure = 0, kPhLin = 1, kPhSchur = 2, kPhLdlt = 3, kPhUpdate = 4 };

struct IbaRun {
  inertial_ba_handle* const h;
  const hipStream_t st;
  const inertial_ba_problem* const p;
  inertial_ba_result* const r;
  StopCheck stop;                      // (no flag: LocalInertialBA hands its flag to the optimizer after optimize() has returned)
  LmScalars lm;
  IbaCam cam;
  double dM, dS;
  int NK, NX, NE, nF, n, nIE = 0, nbe = 0, n_pairs = 0;
  int cur = 0;
  double last_chi2 = 0;                // of the last evaluation: a rejected trial's if the run ends on one
  // offsets of the tables inside d_ints
  int o_kf_col = 0, o_col_off = 0, o_col_dim = 0, o_pt_start = 0, o_pt_end = 0, o_row_start = 0, o_row_edges = 0, o_pair_i = 0, o_pair_j = 0,
      o_item_start = 0, o_pie_start = 0;

  IbaRun(inertial_ba_handle* h_, const inertial_ba_problem* p_, inertial_ba_result* r_, int nF_, int n_)
      : h(h_), st(h_->stream), p(p_), r(r_), NK(p_->n_keyframes), NX(p_->n_points), NE(p_->n_edges), nF(nF_), n(n_) {
    iba_fill_cam(p, &cam);
    dM = (float)std::sqrt(5.991); dS = (float)std::sqrt(7.815);        // thHuberMono / thHuberStereo are const float (S/Optimizer.cc:4894-4896)
    nbe = (NE + kIbaThreads - 1) / kIbaThreads;
  }
  const int* tab(int off) const { return h->d_ints.p + off; }

  // ---- the structure of the system, on the host
  void structure() {
    std::vector<int>& T = h->s_ints;
    T.clear();
    auto room = [&](size_t cnt) { const int o = (int)T.size(); T.resize(T.size() + cnt, 0); return o; };
    h->s_kfs.resize((size_t)NK);
    o_kf_col = room((size_t)NK); o_col_off = room((size_t)nF); o_col_dim = room((size_t)nF);
    int c = 0, off = 0;
    for (int i = 0; i < NK; i++) {
      const inertial_ba_keyframe& kf = p->keyframes[i];
      iba_widen_state(kf.state, &h->s_kfs[i]);
      if (kf.fixed) { T[o_kf_col + i] = -1; continue; }
      T[o_kf_col + i] = c; T[o_col_off + c] = off; T[o_col_dim + c] = kf.imu ? 15 : 6;
      off += kf.imu ? 15 : 6; c++;
    }
    h->s_points.resize(3 * (size_t)std::max(NX, 1));
    for (size_t i = 0; i < 3 * (size_t)NX; i++) h->s_points[i] = p->points[i];
    // the inertial edges, in keyframe order
    h->s_ies.clear(); h->s_ieP.clear();
    for (int i = 0; i < NK; i++) {
      const inertial_ba_keyframe& kf = p->keyframes[i];
      if (!kf.link) continue;
      h->s_ies.push_back(IbaInertial{kf.prev, i, (kf.last_in_window || p->rec_init) ? 1 : 0, 0});
      h->s_ieP.emplace_back();
      iba_fill_inertial(kf, &h->s_ieP.back());
    }
    nIE = (int)h->s_ies.size();
    // the run of edges of every point, the edges of every free keyframe
    o_pt_start = room((size_t)std::max(NX, 1)); o_pt_end = room((size_t)std::max(NX, 1));
    o_row_start = room((size_t)nF + 1);
    std::vector<int> cnt((size_t)nF, 0);
    for (int k = 0; k < NE; k++) {
      const lba_edge& e = p->edges[k];
      if (k == 0 || p->edges[k - 1].point != e.point) T[o_pt_start + e.point] = k;
      T[o_pt_end + e.point] = k + 1;
      const int col = T[o_kf_col + e.pose];
      if (col >= 0) cnt[col]++;
    }
    for (int i = 0; i < nF; i++) T[o_row_start + i + 1] = T[o_row_start + i] + cnt[i];
    const int n_row_edges = T[o_row_start + nF];
    o_row_edges = room((size_t)std::max(n_row_edges, 1));
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int k = 0; k < NE; k++) {
      const int col = T[o_kf_col + p->edges[k].pose];
      if (col >= 0) { T[o_row_edges + T[o_row_start + col] + cnt[col]] = k; cnt[col]++; }
    }
    // the non-empty pairs: a common landmark or an inertial edge; the diagonal pair exists for every free keyframe
    std::vector<uint8_t> mark((size_t)nF * nF, 0);
    for (int i = 0; i < nF; i++) mark[(size_t)i * nF + i] = 1;
    for (int l = 0; l < NX; l++) {
      const int b = T[o_pt_start + l], e = T[o_pt_end + l];
      for (int a = b; a < e; a++) {
        const int ca = T[o_kf_col + p->edges[a].pose];
        if (ca < 0) continue;
        for (int k = a + 1; k < e; k++) {
          const int cb = T[o_kf_col + p->edges[k].pose];
          if (cb >= 0) mark[(size_t)std::min(ca, cb) * nF + std::max(ca, cb)] = 1;
        }
      }
    }
    for (const IbaInertial& ie : h->s_ies) {
      const int ca = T[o_kf_col + ie.k1], cb = T[o_kf_col + ie.k2];
      if (ca >= 0 && cb >= 0) mark[(size_t)std::min(ca, cb) * nF + std::max(ca, cb)] = 1;
    }
    n_pairs = 0;
    for (uint8_t m : mark) n_pairs += m;
    o_pair_i = room((size_t)n_pairs); o_pair_j = room((size_t)n_pairs);
    o_item_start = room((size_t)n_pairs + 1); o_pie_start = room((size_t)n_pairs + 1);
    h->s_items.clear(); h->s_pies.clear();
    int q = 0;
    for (int i = 0; i < nF; i++)
      for (int j = i; j < nF; j++) {
        if (!mark[(size_t)i * nF + j]) continue;
        T[o_pair_i + q] = i; T[o_pair_j + q] = j;
        T[o_item_start + q] = (int)h->s_items.size(); T[o_pie_start + q] = (int)h->s_pies.size();
        for (int s = T[o_row_start + i]; s < T[o_row_start + i + 1]; s++) {
          const int ea = T[o_row_edges + s];
          if (i == j) { h->s_items.push_back(SchurItem{ea, ea}); continue; }
          const int l = p->edges[ea].point;
          for (int k = T[o_pt_start + l]; k < T[o_pt_end + l]; k++)
            if (T[o_kf_col + p->edges[k].pose] == j) { h->s_items.push_back(SchurItem{ea, k}); break; }
        }
        for (int e = 0; e < nIE; e++) {
          const int ca = T[o_kf_col + h->s_ies[e].k1], cb = T[o_kf_col + h->s_ies[e].k2];
          if (i == j) {
            if (ca == i) h->s_pies.push_back(IbaPairInertial{e, 0, 0});
            if (cb == i) h->s_pies.push_back(IbaPairInertial{e, 15, 15});
          } else if (ca == i && cb == j) h->s_pies.push_back(IbaPairInertial{e, 0, 15});
          else if (ca == j && cb == i) h->s_pies.push_back(IbaPairInertial{e, 15, 0});
        }
        q++;
      }
    T[o_item_start + n_pairs] = (int)h->s_items.size(); T[o_pie_start + n_pairs] = (int)h->s_pies.size();
  }

  int buffers() {
    int rc;
    const size_t sNK = (size_t)NK, sNX = (size_t)std::max(NX, 1), sNE = (size_t)std::max(NE, 1), snF = (size_t)nF, sIE = (size_t)std::max(nIE, 1);
    for (int b = 0; b < 2; b++)
      if ((rc = h->d_kfs[b].reserve(sNK)) || (rc = h->d_points[b].reserve(3 * sNX))) return rc;
    if ((rc = h->d_edges.reserve(sNE)) || (rc = h->d_ints.reserve(h->s_ints.size())) || (rc = h->d_items.reserve(std::max<size_t>(h->s_items.size(), 1))) ||
        (rc = h->d_pies.reserve(std::max<size_t>(h->s_pies.size(), 1))) || (rc = h->d_ies.reserve(sIE)) || (rc = h->d_ieP.reserve(sIE)) ||
        (rc = h->d_chi2.reserve(sNE)) || (rc = h->d_partial.reserve((size_t)std::max(nbe + nIE, 1))) || (rc = h->d_EB.reserve(sNE * kIbaEB)) ||
        (rc = h->d_IEB.reserve(sIE * kIbaIB)) || (rc = h->d_Hll.reserve(6 * sNX)) || (rc = h->d_bl.reserve(3 * sNX)) ||
        (rc = h->d_Hpp.reserve(21 * snF)) || (rc = h->d_bp.reserve(6 * snF)) || (rc = h->d_Dinv.reserve(6 * sNX)) || (rc = h->d_Db.reserve(3 * sNX)) ||
        (rc = h->d_bs.reserve((size_t)n)) || (rc = h->d_bk.reserve((size_t)n)) || (rc = h->d_x.reserve((size_t)n)) ||
        (rc = h->d_scale_v.reserve(sNK + sNX)) || (rc = h->d_depth.reserve(sNE)) || (rc = h->d_ok.reserve(4)) || (rc = h->d_rec.reserve(1)) ||
        (rc = h->rec.reserve(1)))
      return rc;
    return h->ldlt.plan(n, st);
  }

  int upload() {
    // (pageable sources: hipMemcpyAsync returns once the bytes are staged, the host arrays may be reused afterwards)
    ORBG_HIP(hipMemcpyAsync(h->d_kfs[0].p, h->s_kfs.data(), sizeof(PiState) * (size_t)NK, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_ints.p, h->s_ints.data(), sizeof(int) * h->s_ints.size(), hipMemcpyHostToDevice, st));
    if (NX > 0) ORBG_HIP(hipMemcpyAsync(h->d_points[0].p, h->s_points.data(), sizeof(double) * 3 * (size_t)NX, hipMemcpyHostToDevice, st));
    if (NE > 0) ORBG_HIP(hipMemcpyAsync(h->d_edges.p, p->edges, sizeof(lba_edge) * (size_t)NE, hipMemcpyHostToDevice, st));
    if (!h->s_items.empty()) ORBG_HIP(hipMemcpyAsync(h->d_items.p, h->s_items.data(), sizeof(SchurItem) * h->s_items.size(), hipMemcpyHostToDevice, st));
    if (!h->s_pies.empty()) ORBG_HIP(hipMemcpyAsync(h->d_pies.p, h->s_pies.data(), sizeof(IbaPairInertial) * h->s_pies.size(), hipMemcpyHostToDevice, st));
    if (nIE > 0) {
      ORBG_HIP(hipMemcpyAsync(h->d_ies.p, h->s_ies.data(), sizeof(IbaInertial) * (size_t)nIE, hipMemcpyHostToDevice, st));
      ORBG_HIP(hipMemcpyAsync(h->d_ieP.p, h->s_ieP.data(), sizeof(PiParams) * (size_t)nIE, hipMemcpyHostToDevice, st));
    }
    ORBG_HIP(hipStreamSynchronize(st));
    return ORBG_OK;
  }

  // the record of the last launches, on the host
  int fetch_record() {
    const int rc = lm_fetch_record(h->rec.h, h->d_rec.p, st, h->timer);
    if (!rc) last_chi2 = h->rec.h->chi2;
    return rc;
  }

  void launch_edges(int buf, bool lin) {
    if (nbe + nIE > 0)
      hipLaunchKernelGGL(k_iba_edges, dim3(nbe + nIE), dim3(kIbaThreads), 0, st, NE, nbe, h->d_edges.p, h->d_kfs[buf].p, h->d_points[buf].p, cam, dM, dS,
                         h->d_ies.p, h->d_ieP.p, h->d_chi2.p, h->d_partial.p, lin ? h->d_EB.p : (double*)nullptr, lin ? h->d_IEB.p : (double*)nullptr);
  }

  // computeActiveErrors + buildSystem of the current state
  int linearise() {
    h->timer.begin(kPhLin, st);
    launch_edges(cur, true);
    if (NX > 0)
      hipLaunchKernelGGL(k_schur_points<kIbaEB>, dim3((NX + 255) / 256), dim3(256), 0, st, NX, tab(o_pt_start), tab(o_pt_end), h->d_EB.p, h->d_Hll.p, h->d_bl.p);
    hipLaunchKernelGGL(k_iba_poses, dim3(nF), dim3(256), 0, st, tab(o_row_start), tab(o_row_edges), h->d_EB.p, h->d_Hpp.p, h->d_bp.p);
    hipLaunchKernelGGL(k_iba_finish, dim3(1), dim3(256), 0, st, nbe + nIE, h->d_partial.p, 0, h->d_scale_v.p, (const int*)nullptr, h->d_rec.p);
    h->timer.end(st);
    return fetch_record();
  }

  // one trial: solve with lambda, trial state into buffer cur ^ 1, its evaluation
  int trial(double lambda) {
    const int from = cur, to = cur ^ 1;
    int rc;
    h->timer.begin(kPhSchur, st);
    if (NX > 0)
      hipLaunchKernelGGL(k_schur_dinv, dim3((NX + 255) / 256), dim3(256), 0, st, NX, h->d_Hll.p, h->d_bl.p, lambda, h->d_Dinv.p, h->d_Db.p);
    if ((rc = h->ldlt.clear(h->d_x.p, st))) return rc;
    hipLaunchKernelGGL(k_iba_schur, dim3(n_pairs), dim3(256), 0, st, n, tab(o_pair_i), tab(o_pair_j), tab(o_col_off), tab(o_col_dim), tab(o_item_start),
                       h->d_items.p, tab(o_pie_start), h->d_pies.p, h->d_edges.p, h->d_EB.p, h->d_IEB.p, h->d_Dinv.p, h->d_Db.p, h->d_Hpp.p, h->d_bp.p,
                       lambda, h->ldlt.S(), h->d_bs.p, h->d_bk.p, h->ldlt.St());
    h->timer.end(st);
    h->timer.begin(kPhLdlt, st);
    if ((rc = h->ldlt.launch(h->d_bs.p, h->d_x.p, h->d_ok.p, st))) return rc;
    h->timer.end(st);
    h->timer.begin(kPhUpdate, st);
    hipLaunchKernelGGL(k_iba_update, dim3((NK + NX + 255) / 256), dim3(256), 0, st, NK, NX, tab(o_kf_col), tab(o_col_off), tab(o_col_dim),
                       h->d_kfs[from].p, h->d_points[from].p, h->d_x.p, tab(o_pt_start), tab(o_pt_end), h->d_edges.p, h->d_EB.p, h->d_Dinv.p, h->d_bl.p,
                       h->d_bk.p, lambda, h->d_ok.p, h->d_kfs[to].p, h->d_points[to].p, h->d_scale_v.p);
    launch_edges(to, false);
    hipLaunchKernelGGL(k_iba_finish, dim3(1), dim3(256), 0, st, nbe + nIE, h->d_partial.p, NK + NX, h->d_scale_v.p, h->d_ok.p, h->d_rec.p);
    h->timer.end(st);
    return fetch_record();
  }

  // ---- what lm_optimize (lm_driver.hpp) asks of a solve
  const LmRec& record() const { return *h->rec.h; }
  int timed_out() const { return ldlt_timed_out_rc(h->rec.h->ok); }
  void accept() { cur ^= 1; }
  int first_linearisation(double* user_lambda) {
    *user_lambda = p->large ? 1e-2 : 1e0;          // setUserLambdaInit (S/Optimizer.cc:4690-4701)
    r->chi2_initial = lm.currentChi;               // computeActiveErrors(); err = activeRobustChi2() in front of optimize()
    return ORBG_OK;
  }
  void iteration_done(int qmax, bool) { lm_trace_row(lm, qmax, r->trace, r->trace_cap, &r->trace_len); }

  // ---- results: chi2 of the LAST error evaluation, depth test and states of the final estimate, the verdicts
  int download() {
    if (NE > 0) {
      hipLaunchKernelGGL(k_iba_depth, dim3(nbe), dim3(256), 0, st, NE, h->d_edges.p, h->d_kfs[cur].p, h->d_points[cur].p, cam, h->d_depth.p);
      ORBG_HIP(hipGetLastError());
    }
    std::vector<double> chi2((size_t)NE);
    std::vector<uint8_t> depth((size_t)NE);
    if (NE > 0) {
      ORBG_HIP(hipMemcpyAsync(depth.data(), h->d_depth.p, (size_t)NE, hipMemcpyDeviceToHost, st));
      ORBG_HIP(hipMemcpyAsync(chi2.data(), h->d_chi2.p, sizeof(double) * (size_t)NE, hipMemcpyDeviceToHost, st));
    }
    ORBG_HIP(hipMemcpyAsync(h->s_kfs.data(), h->d_kfs[cur].p, sizeof(PiState) * (size_t)NK, hipMemcpyDeviceToHost, st));
    if (NX > 0) ORBG_HIP(hipMemcpyAsync(h->s_points.data(), h->d_points[cur].p, sizeof(double) * 3 * (size_t)NX, hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < NK; i++) {
      const PiState& s = h->s_kfs[i];
      inertial_ba_state& o = r->states[i];
      memcpy(o.Rwb, s.R, sizeof(o.Rwb)); memcpy(o.twb, s.t, sizeof(o.twb)); memcpy(o.vwb, s.v, sizeof(o.vwb));
      memcpy(o.bg, s.bg, sizeof(o.bg)); memcpy(o.ba, s.ba, sizeof(o.ba));
    }
    for (size_t i = 0; i < 3 * (size_t)NX; i++) r->points[i] = (float)h->s_points[i];
    // S/Optimizer.cc:5088-5119: double chi2 against widened floats; 1.5f * chi2Mono2 is a float product
    const float chi2Mono2 = 5.991f, chi2Stereo2 = 7.815f;
    const float chi2Close = 1.5f * chi2Mono2;
    int n_out = 0;
    for (int k = 0; k < NE; k++) {
      const lba_edge& e = p->edges[k];
      bool out;
      if (e.ur < 0) {
        const bool close = p->close[e.point] != 0;
        out = (chi2[k] > chi2Mono2 && !close) || (chi2[k] > chi2Close && close) || !depth[k];
      } else out = chi2[k] > chi2Stereo2;
      n_out += out ? 1 : 0;
      if (r->edge_chi2) r->edge_chi2[k] = chi2[k];
      if (r->edge_depth_pos) r->edge_depth_pos[k] = depth[k];
      if (r->edge_outlier) r->edge_outlier[k] = out ? 1 : 0;
    }
    r->n_outliers = n_out;
    r->chi2_final = last_chi2;                     // err_end = activeRobustChi2(): the errors of the last evaluation
    const float err = (float)r->chi2_initial, err_end = (float)r->chi2_final;
    r->failed = ((2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !p->large) ? 1 : 0;      // :5128
    return ORBG_OK;
  }
};

int iba_attempt(inertial_ba_handle* h, const inertial_ba_problem* p, inertial_ba_result* r, int nF, int n) {
  IbaRun run(h, p, r, nF, n);
  int rc;
  r->iters = 0; r->trace_len = 0; r->chi2_initial = r->chi2_final = 0; r->n_outliers = 0; r->failed = 0;
  if ((rc = select_device(h->device))) return rc;
  if ((rc = h->timer.reset())) return rc;
  StreamDrain drain{h->stream};
  h->timer.begin(kPhStructure, h->stream);
  run.structure();
  if ((rc = run.buffers()) || (rc = run.upload())) return rc;
  h->timer.end(h->stream);
  int done = 0;
  if ((rc = lm_optimize(run, p->large ? 4 : 10, run.stop, &done))) return rc;
  r->iters = done;
  rc = run.download();
  h->timer.flush(h->stream);
  return rc;
}

int iba_solve_impl(inertial_ba_handle* h, const inertial_ba_problem* p, inertial_ba_result* r, int nF = -1, int n = 0) {
  if (!h) return ORBG_BAD_ARG;
  int rc;
  if (nF < 0 && (rc = iba_validate(p, r, &nF, &n))) return rc;
  // (a timed-out launch: solved again on the one-workgroup kernels, which this handle then keeps using)
  return ldlt_retry(h->ldlt, h->stream, [&] { return iba_attempt(h, p, r, nF, n); });
}

}  // namespace

extern "C" int inertial_ba_create(int device, inertial_ba_handle** out) {
  if (!out) return ORBG_BAD_ARG;
  int rc = select_device(device);
  if (rc) return rc;
  inertial_ba_handle* h = new inertial_ba_handle();
  h->device = device;
  h->ldlt.read_env();
  if (orbg::create_stream(&h->stream, "lba") != hipSuccess) { delete h; return ORBG_HIP_ERROR; }
  *out = h;
  return ORBG_OK;
}

extern "C" int inertial_ba_destroy(inertial_ba_handle* h) {
  if (!h) return ORBG_BAD_ARG;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->ldlt.release();
  h->d_edges.release();
  for (int i = 0; i < 2; i++) { h->d_kfs[i].release(); h->d_points[i].release(); }
  h->d_ints.release(); h->d_ok.release(); h->d_items.release(); h->d_pies.release(); h->d_ies.release(); h->d_ieP.release();
  for (DevBuf<double>* b : {&h->d_chi2, &h->d_partial, &h->d_EB, &h->d_IEB, &h->d_Hll, &h->d_bl, &h->d_Hpp, &h->d_bp, &h->d_Dinv, &h->d_Db, &h->d_bs,
                            &h->d_bk, &h->d_x, &h->d_scale_v})
    b->release();
  h->d_depth.release(); h->d_rec.release(); h->rec.release();
  h->timer.release();
  if (!h->ext_stream) orbg::release_stream(h->stream);
  delete h;
  return ORBG_OK;
}

extern "C" int inertial_ba_set_stream(inertial_ba_handle* h, void* hip_stream) {
  if (!h) return ORBG_BAD_ARG;
  int rc = select_device(h->device);
  if (rc) return rc;
  return orbg::swap_stream(&h->stream, &h->ext_stream, hip_stream, "lba");
}

extern "C" int inertial_ba_solve_h(inertial_ba_handle* h, const inertial_ba_problem* p, inertial_ba_result* r) { return iba_solve_impl(h, p, r); }

extern "C" int inertial_ba_solve(const inertial_ba_problem* p, inertial_ba_result* r) {
  int nF = 0, n = 0;
  int rc = iba_validate(p, r, &nF, &n);            // refusals come before a handle (a device, a stream) exists
  if (rc) return rc;
  inertial_ba_handle* h = nullptr;
  if ((rc = inertial_ba_create(p->device, &h))) return rc;
  rc = iba_solve_impl(h, p, r, nF, n);
  inertial_ba_destroy(h);
  return rc;
}

extern "C" int inertial_ba_set_profiling(inertial_ba_handle* h, int on) {
  if (!h) return ORBG_BAD_ARG;
  h->timer.on = on != 0;
  return ORBG_OK;
}
extern "C" int inertial_ba_get_phase_ms(inertial_ba_handle* h, double* ms) {
  if (!h || !ms) return ORBG_BAD_ARG;
  for (int i = 0; i < 5; i++) ms[i] = h->timer.ms[i];
  return ORBG_OK;
}

// TEST AID (include/orbgpu.h): the edge arithmetic of the kernels, compiled for the host, at the estimates handed in
extern "C" int inertial_ba_host_linearize(const inertial_ba_problem* p, double* vis, double* inertial) {
  if (!p || p->struct_size < sizeof(inertial_ba_problem)) return ORBG_BAD_ARG;
  if (p->n_keyframes <= 0 || !p->keyframes || p->n_edges < 0 || p->n_points < 0) return ORBG_BAD_ARG;
  if (p->n_edges > 0 && (!p->edges || !p->points || !vis)) return ORBG_BAD_ARG;
  IbaCam C;
  iba_fill_cam(p, &C);
  std::vector<PiState> kfs((size_t)p->n_keyframes);
  for (int i = 0; i < p->n_keyframes; i++) iba_widen_state(p->keyframes[i].state, &kfs[i]);
  for (int k = 0; k < p->n_edges; k++) {
    const lba_edge& e = p->edges[k];
    if (e.pose < 0 || e.pose >= p->n_keyframes || e.point < 0 || e.point >= p->n_points || iba_edge_is_right(e.ur)) return ORBG_BAD_ARG;
    double cam[12], X[3], Jl[9], Jp[18];
    pi_camera_pose(kfs[e.pose], C.Rcb, C.tcb, cam);
    for (int i = 0; i < 3; i++) X[i] = p->points[3 * (size_t)e.point + i];
    IbaVis o;
    iba_visual_error(cam, C, X, e.u, e.v, e.ur, (double)e.inv_sigma2, &o);
    iba_visual_jacobians(o, cam, C, e.ur < 0, Jl, Jp);
    double* out = vis + 31 * (size_t)k;
    for (int i = 0; i < 3; i++) out[i] = o.e[i];
    out[3] = o.c2;
    for (int i = 0; i < 9; i++) out[4 + i] = Jl[i];
    for (int i = 0; i < 18; i++) out[13 + i] = Jp[i];
  }
  int ne = 0;
  for (int i = 0; i < p->n_keyframes; i++) {
    const inertial_ba_keyframe& kf = p->keyframes[i];
    if (!kf.link) continue;
    if (kf.prev < 0 || kf.prev >= p->n_keyframes || !inertial) return ORBG_BAD_ARG;
    static thread_local PiParams P;
    iba_fill_inertial(kf, &P);
    double* J = inertial + (size_t)ne * 15 * kPiLd;
    for (int q = 0; q < 15 * kPiLd; q++) J[q] = 0;
    pi_inertial_edge(P, kfs[kf.prev], kfs[i], true, 15, 30, J);
    iba_walk_edges(kfs[kf.prev], kfs[i], J);
    ne++;
  }
  return ORBG_OK;
}
