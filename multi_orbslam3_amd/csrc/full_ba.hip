// liborbgpu -- full bundle adjustment for gfx950 (MI355X).  Replaces the numerical core of Optimizer::BundleAdjustment
// (S/Optimizer.cc:73-446, reached through GlobalBundleAdjustemnt from Tracking::CreateInitialMapMonocular and
// LoopClosing::RunGlobalBundleAdjustment) behind ba_solve() of include/orbgpu.h: ONE optimize(nIterations) over every keyframe and
// map point of a map, Huber kernels on or off, every edge with the camera of its own keyframe.
//
// The edges, the Huber kernel, the LM decisions and the LDL^T solvers are the local BA's (ba_edge.hpp, lm_step.hpp behind lm_driver.hpp,
// ldlt_mfma.hpp, ldlt_xcd.hpp, ldlt_wide.hpp); the landmark-Schur arithmetic between them (landmark_schur.hpp) and the record of an evaluation
// (lm_record.hpp) are shared with inertial_ba.hip.  What is new is everything whose size goes with the MAP instead of a window (DESIGN.md,
// "BundleAdjustment"): hundreds of free poses, 10^5 .. 10^6 edges, a reduced camera system most of whose blocks are empty.
//   structure, once per call, all on the device, no sort and no floating-point atomic:
//     k_ba_ranges                 the run of edges of every point (a point's edges are consecutive)
//     k_ba_tile_count/scan/place  the edges of every free pose in ascending order: a stable counting sort over tiles of edges
//     k_ba_pair_mark/count/emit   which pose pairs share a landmark: a bitmap (integer OR), compacted row by row in ascending order
//     k_ba_items_count/fill       per non-empty pair the (edge of i, edge of j) items of the landmarks both observe, in the order of
//                                 pose i's edge list (ordered compaction)
//   per LM iteration:
//     k_ba_lin      thread/edge  residual, chi2, rho, Jacobians -> Hpl | Hll | bl blocks
//     k_schur_points thread/point Hll, bl in edge order;  k_ba_poses  workgroup/free pose  Hpp, bp (fixed tree)
//   per trial:
//     k_schur_dinv  thread/point (Hll + lambda I)^-1 and its product with bl
//     one fill of the dense reduced system, then k_ba_schur: workgroup per NON-EMPTY pair, items in fixed order
//     LDL^T by size (<= 20 free poses: one workgroup on the matrix cores, <= 50: eight workgroups, beyond: k_wide_*)
//     k_ba_update   thread/vertex  back-substitution, trial state, computeScale terms
//     k_ba_errors + k_ba_finish   robust chi2, scale, largest diagonal -> the record the host reads
// Every sum has a fixed order: two calls on the same input return the same bits.
//
// ba_weld_solve() is the welding BA of LoopClosing::MergeLocal (Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, ...),
// S/Optimizer.cc:6305-6983) on the same run: round 1 is the solve above with kernels on, then on the device
//     k_ba_weld_classify  thread/edge  level by chi2 threshold and depth test; k_ba_scan of the keep flags;
//     k_ba_weld_compact   thread/edge  the level-0 edges, in order, into a second edge list + their origins
// round 2 = structure + optimize over that list with kernels off, and k_ba_weld_scatter puts its chi2 back into the full list.

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

#include "se3.hpp"
#include "lm_driver.hpp"
#include "lm_record.hpp"

using namespace orbg;
using namespace orbg_se3;
using namespace orbg_lm;

namespace {

// The solvers' kernels are ordinary (non-template) __global__ functions: a second translation unit that includes them needs copies
// of its own.  Everything these headers include themselves is already included above, so only their own declarations land here.
#include "ldlt_mfma.hpp"
#include "ldlt_xcd.hpp"
#include "ba_edge.hpp"
#include "ldlt_wide.hpp"
#include "ldlt_solver.hpp"
#include "landmark_schur.hpp"

constexpr int kEB = 27;                 // per-edge blocks: Hpl (6x3, 18) | Hll upper (6) | bl (3), as in lba.hip
static_assert(kEB == kSchurHead, "an edge's block is exactly what landmark_schur.hpp reads: Hpl | Hll | bl");
constexpr int kMaxCols = BA_MAX_FREE_POSES;
constexpr int kTileEdges = 256;         // edges per workgroup pass of the counting sort
constexpr int kMaxTiles = 2048;

// ------------------------------------------------------------------------------------------ structure

__global__ __launch_bounds__(256) void k_ba_ranges(int NE, const lba_edge* __restrict__ edges, int* __restrict__ pt_start, int* __restrict__ pt_end) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= NE) return;
  const int p = edges[k].point;
  if (k == 0 || edges[k - 1].point != p) pt_start[p] = k;
  if (k == NE - 1 || edges[k + 1].point != p) pt_end[p] = k + 1;
}

// exclusive scan of n ints by ONE workgroup of 1024 threads: out[0 .. n], *total = out[n] in 64 bits
__global__ __launch_bounds__(1024) void k_ba_scan(int n, const int* __restrict__ in, int* __restrict__ out, long long* __restrict__ total) {
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const int chunk = (n + 1023) / 1024;
  const int b = min(n, tid * chunk), e = min(n, b + chunk);
  long long s = 0;
  for (int i = b; i < e; i++) s += in[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < 1024; i++) { const long long v = part[i]; part[i] = run; run += v; }
    *total = run;
    out[n] = run > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)run;
  }
  __syncthreads();
  long long run = part[tid];
  for (int i = b; i < e; i++) { const int v = in[i]; out[i] = run > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)run; run += v; }
}

// tile t = edges [t * tile, (t + 1) * tile): how many edges of every free pose it holds
__global__ __launch_bounds__(256) void k_ba_tile_count(int NE, int tile, const lba_edge* __restrict__ edges, const int* __restrict__ pose_col,
                                                       int nP, int* __restrict__ table) {
  __shared__ int hist[kMaxCols];
  for (int c = threadIdx.x; c < nP; c += 256) hist[c] = 0;
  __syncthreads();
  const long long b = (long long)blockIdx.x * tile;
  const int e = (int)min((long long)NE, b + tile);
  for (int k = (int)b + threadIdx.x; k < e; k += 256) {
    const int c = pose_col[edges[k].pose];
    if (c >= 0) atomicAdd(&hist[c], 1);            // integer count: order does not matter
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nP; c += 256) table[(size_t)blockIdx.x * nP + c] = hist[c];
}
// per free pose: counts -> offsets of the tiles inside the pose's list; the pose's degree
__global__ __launch_bounds__(256) void k_ba_tile_scan(int n_tiles, int nP, int* __restrict__ table, int* __restrict__ row_count) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nP) return;
  int run = 0;
  for (int t = 0; t < n_tiles; t++) { const int v = table[(size_t)t * nP + c]; table[(size_t)t * nP + c] = run; run += v; }
  row_count[c] = run;
}
// every edge to its place: row_start[col] + offset of the tile + rank among the tile's earlier edges of that pose
__global__ __launch_bounds__(256) void k_ba_tile_place(int NE, int tile, const lba_edge* __restrict__ edges, const int* __restrict__ pose_col,
                                                       int nP, const int* __restrict__ table, const int* __restrict__ row_start,
                                                       int* __restrict__ row_edges) {
  __shared__ int run[kMaxCols];
  __shared__ int cols[256];
  const int tid = threadIdx.x;
  for (int c = tid; c < nP; c += 256) run[c] = row_start[c] + table[(size_t)blockIdx.x * nP + c];
  const long long b = (long long)blockIdx.x * tile;
  const int e = (int)min((long long)NE, b + tile);
  for (int k0 = (int)b; k0 < e; k0 += 256) {
    const int k = k0 + tid;
    const int c = k < e ? pose_col[edges[k].pose] : -1;
    __syncthreads();                               // run[] of the previous pass (or its initialisation) is complete
    cols[tid] = c;
    __syncthreads();
    int pos = -1;
    bool last = true;
    if (c >= 0) {
      int rank = 0;
      for (int t = 0; t < tid; t++) rank += cols[t] == c ? 1 : 0;
      for (int t = tid + 1; t < 256; t++) if (cols[t] == c) { last = false; break; }
      pos = run[c] + rank;
      row_edges[pos] = k;
    }
    __syncthreads();                               // every read of run[] is done
    if (c >= 0 && last) run[c] = pos + 1;
  }
}

// the edge of point l's run that observes free pose column j, or -1
__device__ __forceinline__ int find_obs(int b, int e, int j, const lba_edge* __restrict__ edges, const int* __restrict__ pose_col) {
  for (int k = b; k < e; k++) if (pose_col[edges[k].pose] == j) return k;
  return -1;
}

// bit (i, j), i < j, of the pair bitmap: free poses i and j observe a common landmark
__global__ __launch_bounds__(256) void k_ba_pair_mark(int NX, const int* __restrict__ pt_start, const int* __restrict__ pt_end,
                                                      const lba_edge* __restrict__ edges, const int* __restrict__ pose_col, int W,
                                                      unsigned* __restrict__ bitmap) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= NX) return;
  const int b = pt_start[l], e = pt_end[l];
  for (int a = b; a < e; a++) {
    const int ca = pose_col[edges[a].pose];
    if (ca < 0) continue;
    for (int k = a + 1; k < e; k++) {
      const int cb = pose_col[edges[k].pose];
      if (cb < 0 || cb == ca) continue;
      const int i = min(ca, cb), j = max(ca, cb);
      atomicOr(&bitmap[(size_t)i * W + (j >> 5)], 1u << (j & 31));   // idempotent
    }
  }
}
__global__ __launch_bounds__(256) void k_ba_pair_count(int nP, int W, const unsigned* __restrict__ bitmap, int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nP) return;
  int n = 1;                                       // the diagonal pair exists for every free pose
  for (int w = 0; w < W; w++) n += __popc(bitmap[(size_t)i * W + w]);
  cnt[i] = n;
}
__global__ __launch_bounds__(256) void k_ba_pair_emit(int nP, int W, const unsigned* __restrict__ bitmap, const int* __restrict__ pair_row_start,
                                                      int* __restrict__ pair_i, int* __restrict__ pair_j) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nP) return;
  int o = pair_row_start[i];
  pair_i[o] = i; pair_j[o] = i; o++;
  for (int w = 0; w < W; w++) {
    unsigned m = bitmap[(size_t)i * W + w];
    while (m) { const int bit = __ffs((int)m) - 1; m &= m - 1; pair_i[o] = i; pair_j[o] = 32 * w + bit; o++; }
  }
}
// items of pair (i, j): the edges of pose i's list whose landmark pose j observes too
__global__ __launch_bounds__(256) void k_ba_items_count(int n_pairs, const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                        const int* __restrict__ row_start, const int* __restrict__ row_edges,
                                                        const lba_edge* __restrict__ edges, const int* __restrict__ pt_start,
                                                        const int* __restrict__ pt_end, const int* __restrict__ pose_col, int* __restrict__ item_cnt) {
  __shared__ int total;
  const int p = blockIdx.x;
  const int i = pair_i[p], j = pair_j[p];
  const int b = row_start[i], e = row_start[i + 1];
  if (i == j) { if (threadIdx.x == 0) item_cnt[p] = e - b; return; }
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int n = 0;
  for (int q = b + threadIdx.x; q < e; q += 256) {
    const int l = edges[row_edges[q]].point;
    n += find_obs(pt_start[l], pt_end[l], j, edges, pose_col) >= 0 ? 1 : 0;
  }
  if (n) atomicAdd(&total, n);
  __syncthreads();
  if (threadIdx.x == 0) item_cnt[p] = total;
}
__global__ __launch_bounds__(256) void k_ba_items_fill(int n_pairs, const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                       const int* __restrict__ row_start, const int* __restrict__ row_edges,
                                                       const lba_edge* __restrict__ edges, const int* __restrict__ pt_start,
                                                       const int* __restrict__ pt_end, const int* __restrict__ pose_col,
                                                       const int* __restrict__ item_start, SchurItem* __restrict__ items) {
  __shared__ int flag[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int i = pair_i[p], j = pair_j[p];
  const int b = row_start[i], e = row_start[i + 1];
  int base = item_start[p];
  if (i == j) {
    for (int q = b + tid; q < e; q += 256) { const int k = row_edges[q]; items[base + (q - b)] = SchurItem{k, k}; }
    return;
  }
  for (int q0 = b; q0 < e; q0 += 256) {
    const int q = q0 + tid;
    int ea = -1, eb = -1;
    if (q < e) {
      ea = row_edges[q];
      const int l = edges[ea].point;
      eb = find_obs(pt_start[l], pt_end[l], j, edges, pose_col);
    }
    __syncthreads();
    flag[tid] = eb >= 0 ? 1 : 0;
    __syncthreads();
    int rank = 0, tot = 0;
    for (int t = 0; t < 256; t++) { const int f = flag[t]; tot += f; if (t < tid) rank += f; }
    if (eb >= 0) items[base + rank] = SchurItem{ea, eb};
    base += tot;
  }
}

// ------------------------------------------------------------------------------------------ per iteration

__device__ __forceinline__ void edge_rho(double chi, bool mono, int robust, const Huber& hb, double* rho0, double* rho1) {
  if (robust) lm_huber(chi, mono ? hb.delta_mono : hb.delta_stereo, mono ? hb.dsqr_mono : hb.dsqr_stereo, rho0, rho1);
  else { *rho0 = chi; *rho1 = 1.0; }
}

// residuals of state (poses, points): chi2 per edge, the workgroup's robust partial
__global__ __launch_bounds__(256) void k_ba_errors(int NE, const lba_edge* __restrict__ edges, const PoseQ* __restrict__ poses,
                                                   const double* __restrict__ points, const int* __restrict__ pose_cam,
                                                   const CamRig* __restrict__ cams, int robust, Huber hb, double* __restrict__ chi2,
                                                   double* __restrict__ partial) {
  __shared__ double red[4];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double rho0 = 0;
  if (k < NE) {
    const lba_edge e = edges[k];
    const PoseQ T = poses[e.pose];
    const double* X = points + 3 * (size_t)e.point;
    double er[3], Xc[3];
    edge_error(T, X, cams[pose_cam[e.pose]], e, er, Xc);
    const bool mono = e.ur < 0;
    const int D = mono ? 2 : 3;
    const double om = (double)e.inv_sigma2;
    double chi = 0, rho1;
    for (int i = 0; i < D; i++) chi += er[i] * (om * er[i]);
    chi2[k] = chi;
    edge_rho(chi, mono, robust, hb, &rho0, &rho1);
  }
  const double s = block_sum_256(rho0, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// computeActiveErrors + the edge part of buildSystem
__global__ __launch_bounds__(256) void k_ba_lin(int NE, const lba_edge* __restrict__ edges, const PoseQ* __restrict__ poses,
                                                const double* __restrict__ points, const int* __restrict__ pose_cam,
                                                const CamRig* __restrict__ cams, int robust, Huber hb, double* __restrict__ chi2,
                                                double* __restrict__ partial, double* __restrict__ EB) {
  __shared__ double red[4];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double rho0 = 0;
  if (k < NE) {
    const lba_edge e = edges[k];
    const PoseQ T = poses[e.pose];
    const double* X = points + 3 * (size_t)e.point;
    const CamRig& g = cams[pose_cam[e.pose]];
    double er[3], Xc[3];
    edge_error(T, X, g, e, er, Xc);
    const bool mono = e.ur < 0;
    const int D = mono ? 2 : 3;
    const double om = (double)e.inv_sigma2;
    double chi = 0, rho1;
    for (int i = 0; i < D; i++) chi += er[i] * (om * er[i]);
    chi2[k] = chi;
    edge_rho(chi, mono, robust, hb, &rho0, &rho1);
    double r[3], A[9], B[18];
    quat_rotate(T.q, X, r);
    edge_jacobians(T, r[0] + T.t[0], r[1] + T.t[1], r[2] + T.t[2], g, e.ur, A, B);
    const double wom = rho1 * om;
    double omega_r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) omega_r[i] = i < D ? -(om * er[i]) * rho1 : 0.0;
    double* out = EB + (size_t)k * kEB;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double h = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) h += B[6 * i + a] * wom * A[3 * i + c];
        out[3 * a + c] = h;
      }
    int o = 18;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b2 = a; b2 < 3; b2++) {
        double h = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) h += A[3 * i + a] * wom * A[3 * i + b2];
        out[o++] = h;
      }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      double s = 0;
#pragma unroll
      for (int i = 0; i < 3; i++) s += A[3 * i + a] * omega_r[i];
      out[o++] = s;
    }
  }
  const double s = block_sum_256(rho0, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Hpp (21 upper entries), bp of one free pose: rebuilt from its edges, thread t takes edges t, t + 256, ... in order
__global__ __launch_bounds__(256) void k_ba_poses(const int* __restrict__ row_start, const int* __restrict__ row_edges,
                                                  const lba_edge* __restrict__ edges, const PoseQ* __restrict__ poses,
                                                  const double* __restrict__ points, const int* __restrict__ pose_cam,
                                                  const CamRig* __restrict__ cams, int robust, Huber hb, const double* __restrict__ chi2,
                                                  double* __restrict__ Hpp, double* __restrict__ bp) {
  const int p = blockIdx.x;
  const int b = row_start[p], e_end = row_start[p + 1];
  double acc[27];
#pragma unroll
  for (int i = 0; i < 27; i++) acc[i] = 0;
  for (int q = b + threadIdx.x; q < e_end; q += 256) {
    const int k = row_edges[q];
    const lba_edge e = edges[k];
    const PoseQ T = poses[e.pose];
    const double* X = points + 3 * (size_t)e.point;
    const CamRig& g = cams[pose_cam[e.pose]];
    double er[3], Xc[3];
    edge_error(T, X, g, e, er, Xc);
    const bool mono = e.ur < 0;
    const int D = mono ? 2 : 3;
    double rho0, rho1;
    edge_rho(chi2[k], mono, robust, hb, &rho0, &rho1);
    double r[3], A[9], B[18];
    quat_rotate(T.q, X, r);
    edge_jacobians(T, r[0] + T.t[0], r[1] + T.t[1], r[2] + T.t[2], g, e.ur, A, B);
    const double om = (double)e.inv_sigma2;
    const double wom = rho1 * om;
    double omega_r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) omega_r[i] = i < D ? -(om * er[i]) * rho1 : 0.0;
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b2 = a; b2 < 6; b2++) {
        double h = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) h += B[6 * i + a] * wom * B[6 * i + b2];
        acc[o++] += h;
      }
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double s = 0;
#pragma unroll
      for (int i = 0; i < 3; i++) s += B[6 * i + a] * omega_r[i];
      acc[o++] += s;
    }
  }
  schur_pose_tail(acc, p, Hpp, bp);
}

// ------------------------------------------------------------------------------------------ per trial

// S_ij = [i == j](Hpp_i + lambda I) - sum_l Hpl_il Dinv_l Hpl_jl^T over the pair's items; diagonal pairs also
// bs_i = bp_i - sum_l Hpl_il (Dinv_l bl_l).  One workgroup per NON-EMPTY pair; blocks of absent pairs keep the zeros of the fill.
__global__ __launch_bounds__(256) void k_ba_schur(int nP, const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                  const int* __restrict__ item_start, const SchurItem* __restrict__ items,
                                                  const lba_edge* __restrict__ edges, const double* __restrict__ EB,
                                                  const double* __restrict__ Dinv, const double* __restrict__ Db,
                                                  const double* __restrict__ Hpp, const double* __restrict__ bp, double lambda,
                                                  double* __restrict__ S, double* __restrict__ bs, double* __restrict__ St) {
  __shared__ double wpart[4][42];
  const int p = blockIdx.x;
  const int i1 = pair_i[p], i2 = pair_j[p];
  const bool diag = i1 == i2;
  const int b = item_start[p], e = item_start[p + 1];
  schur_pair_items<kEB>(diag, b, e, items, edges, EB, Dinv, Db, wpart);
  const int tid = threadIdx.x;
  const int n = 6 * nP;
  // every entry of the system and its mirror image are written by ONE thread, with one value: on a diagonal pair the thread of
  // (a, c), a <= c, alone (the sum of (c, a) is the same number rounded otherwise)
  if (tid < 36) {
    if (diag && tid / 6 > tid % 6) return;
    const double s = ((wpart[0][tid] + wpart[1][tid]) + wpart[2][tid]) + wpart[3][tid];
    const int a = tid / 6, c = tid % 6;
    double v = -s;
    if (diag) {
      const int u = a * 6 - a * (a - 1) / 2 + (c - a);           // index into the 21 upper entries
      v += Hpp[21 * (size_t)i1 + u] + (a == c ? lambda : 0.0);
    }
    const int r = 6 * i1 + a, cc = 6 * i2 + c;
    schur_store_entry(r, cc, n, v, S, St);
  } else if (diag && tid < 42) {
    const int a = tid - 36;
    const double s = ((wpart[0][tid] + wpart[1][tid]) + wpart[2][tid]) + wpart[3][tid];
    const double v = bp[6 * (size_t)i1 + a] - s;
    bs[6 * i1 + a] = v;
    if (St) ldltm::image_put_rhs(St, n, 6 * i1 + a, v);
  }
}

// trial state = oplus(current, x); per vertex its term of computeScale: sum_j x_j (lambda x_j + b_j)
__global__ __launch_bounds__(256) void k_ba_update(int NP, int NX, const int* __restrict__ pose_col, const PoseQ* __restrict__ poses,
                                                   const double* __restrict__ points, const double* __restrict__ x,
                                                   const int* __restrict__ pt_start, const int* __restrict__ pt_end,
                                                   const lba_edge* __restrict__ edges, const double* __restrict__ EB,
                                                   const double* __restrict__ Dinv, const double* __restrict__ bl,
                                                   const double* __restrict__ bp, double lambda, const int* __restrict__ ok_flag,
                                                   PoseQ* __restrict__ poses_out, double* __restrict__ points_out, double* __restrict__ scale_v) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= NP + NX) return;
  const bool ok = *ok_flag != 0;                   // a failed solve leaves no step: the trial state is the current one
  if (v < NP) {
    const int c = pose_col[v];
    double sc = 0;
    if (c < 0 || !ok) poses_out[v] = poses[v];
    else {
      double u[6];
#pragma unroll
      for (int a = 0; a < 6; a++) { u[a] = x[6 * c + a]; sc += u[a] * (lambda * u[a] + bp[6 * (size_t)c + a]); }
      PoseQ T;
      pose_oplus(poses[v], u, &T);
      poses_out[v] = T;
    }
    scale_v[v] = sc;
    return;
  }
  schur_update_point<kEB>(v - NP, ok, pose_col, [](int c) { return 6 * c; }, points, x, pt_start, pt_end, edges, EB, Dinv, bl, lambda, points_out,
                          scale_v + v);
}

// one workgroup: the largest diagonal entry of a linearisation (Hpp given), then lm_finish_record
__global__ __launch_bounds__(256) void k_ba_finish(int n_partial, const double* __restrict__ partial, int n_scale, const double* __restrict__ scale_v,
                                                   int nP, const double* __restrict__ Hpp, int NX, const double* __restrict__ Hll,
                                                   const int* __restrict__ pt_start, const int* __restrict__ pt_end,
                                                   const int* __restrict__ ok_flag, LmRec* __restrict__ rec) {
  const int tid = threadIdx.x;
  double m = 0;
  if (Hpp) {
    for (int i = tid; i < nP; i += 256) {
      const double* h = Hpp + 21 * (size_t)i;
      m = fmax(m, fmax(fmax(fabs(h[0]), fabs(h[6])), fmax(fabs(h[11]), fmax(fabs(h[15]), fmax(fabs(h[18]), fabs(h[20]))))));
    }
    for (int l = tid; l < NX; l += 256) {
      if (pt_end[l] <= pt_start[l]) continue;
      const double* h = Hll + 6 * (size_t)l;
      m = fmax(m, fmax(fabs(h[0]), fmax(fabs(h[3]), fabs(h[5]))));
    }
  }
  lm_finish_record(n_partial, partial, n_scale, scale_v, m, ok_flag, rec);
}

__global__ __launch_bounds__(256) void k_ba_depth(int NE, const lba_edge* __restrict__ edges, const PoseQ* __restrict__ poses,
                                                  const double* __restrict__ points, uint8_t* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= NE) return;
  const lba_edge e = edges[k];
  double rr[3];
  quat_rotate(poses[e.pose].q, points + 3 * (size_t)e.point, rr);
  out[k] = rr[2] + poses[e.pose].t[2] > 0.0 ? 1 : 0;
}

__global__ void k_ba_set_ok(int* ok) { *ok = 1; }

// ------------------------------------------------------------------------------------------ welding BA: between the rounds

// S/Optimizer.cc:6610-6647: level 1 for an edge whose chi2 (of round 1's last evaluation) exceeds its threshold or whose depth is
// not positive at the current estimate; keep = 1 for the edges that stay at level 0
__global__ __launch_bounds__(256) void k_ba_weld_classify(int NE, const lba_edge* __restrict__ edges, const PoseQ* __restrict__ poses,
                                                          const double* __restrict__ points, const double* __restrict__ chi2, double th_mono,
                                                          double th_stereo, uint8_t* __restrict__ level, int* __restrict__ keep) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= NE) return;
  const lba_edge e = edges[k];
  double rr[3];
  quat_rotate(poses[e.pose].q, points + 3 * (size_t)e.point, rr);
  const bool depth_pos = rr[2] + poses[e.pose].t[2] > 0.0;
  const bool out = chi2[k] > (e.ur < 0 ? th_mono : th_stereo) || !depth_pos;
  level[k] = out ? 1 : 0;
  keep[k] = out ? 0 : 1;
}
// the level-0 edges in their order (offset = exclusive scan of keep): a subsequence keeps "the edges of a point are consecutive,
// point never decreases"; origin[j] = the edge compacted edge j came from
__global__ __launch_bounds__(256) void k_ba_weld_compact(int NE, const lba_edge* __restrict__ edges, const int* __restrict__ keep,
                                                         const int* __restrict__ offset, lba_edge* __restrict__ kept, int* __restrict__ origin) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= NE || !keep[k]) return;
  const int j = offset[k];
  kept[j] = edges[k];
  origin[j] = k;
}
// round 2's chi2 back to the full list: the level-1 edges keep round 1's value
__global__ __launch_bounds__(256) void k_ba_weld_scatter(int n_kept, const int* __restrict__ origin, const double* __restrict__ chi2_kept,
                                                         double* __restrict__ chi2) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_kept) return;
  chi2[origin[j]] = chi2_kept[j];
}

}  // namespace

// ---------------------------------------------------------------------------------------------- handle

struct ba_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  LdltSolver ldlt;                     // the solver of the reduced camera system (its switches: read by ba_create)
  DevBuf<lba_edge> d_edges;
  DevBuf<PoseQ> d_poses[2];
  DevBuf<double> d_points[2];
  DevBuf<int> d_pose_col, d_pose_cam, d_pt_start, d_pt_end, d_table, d_row_count, d_row_start, d_row_edges, d_pair_cnt, d_pair_row_start,
      d_pair_i, d_pair_j, d_item_cnt, d_item_start, d_ok;
  DevBuf<unsigned> d_bitmap;
  DevBuf<long long> d_total;
  DevBuf<SchurItem> d_items;
  DevBuf<CamRig> d_cams;
  DevBuf<double> d_chi2, d_partial, d_EB, d_Hll, d_bl, d_Hpp, d_bp, d_Dinv, d_Db, d_bs, d_x, d_scale_v;
  DevBuf<uint8_t> d_depth;
  // welding BA: the level-0 edges and their chi2 (exchanged with d_edges / d_chi2 while round 2 runs), levels, keep flags, their scan, origins
  DevBuf<lba_edge> d_edges_kept;
  DevBuf<double> d_chi2_kept;
  DevBuf<uint8_t> d_level;
  DevBuf<int> d_keep, d_keep_off, d_origin;
  DevBuf<LmRec> d_rec;
  PinnedBuf<LmRec> rec;
  PinnedBuf<long long> total_h;
  std::vector<PoseQ> s_poses;
  std::vector<double> s_points;
  std::vector<int> s_pose_col;
  std::vector<CamRig> s_cams;
  PhaseTimer<5> timer;                 // ba_set_profiling
};

namespace {

enum { kPhStructure = 0, kPhLin = 1, kPhSchur = 2, kPhLdlt = 3, kPhUpdate = 4 };

// What can be refused is refused here, before a device is selected or anything is launched.
int ba_validate(const ba_problem* p, const ba_result* r, int* n_free) {
  if (!p || !r) return ORBG_BAD_ARG;
  if (p->n_poses < 0 || p->n_points < 0 || p->n_edges < 0 || p->n_cameras < 0) return ORBG_BAD_ARG;
  if (!r->poses && p->n_poses > 0) return ORBG_BAD_ARG;
  if (!r->points && p->n_points > 0) return ORBG_BAD_ARG;
  if ((p->n_poses > 0 && (!p->poses || !p->pose_fixed || !p->pose_camera || !p->cameras)) || (p->n_points > 0 && !p->points) ||
      (p->n_edges > 0 && !p->edges))
    return ORBG_BAD_ARG;
  if (p->n_edges > BA_MAX_EDGES) return ORBG_CAP_EXCEEDED;
  int nP = 0;
  for (int i = 0; i < p->n_poses; i++) {
    if (p->pose_camera[i] < 0 || p->pose_camera[i] >= p->n_cameras) return ORBG_BAD_ARG;
    nP += p->pose_fixed[i] ? 0 : 1;
  }
  for (int c = 0; c < p->n_cameras; c++)
    if (p->cameras[c].model.model != ORBG_CAM_PINHOLE && p->cameras[c].model.model != ORBG_CAM_KANNALA_BRANDT8) return ORBG_BAD_ARG;
  if (nP > BA_MAX_FREE_POSES) return ORBG_CAP_EXCEEDED;
  *n_free = nP;
  // the host's one pass over the edges: ranges, the order rule, the right camera's edges (EdgeSE3ProjectXYZToBody: not part of this entry point)
  return schur_check_edges(p->edges, p->n_edges, p->n_poses, p->n_points, [](float ur) { return ur_is_right(ur); });
}

struct BaRun {
  ba_handle* const h;
  const hipStream_t st;
  const ba_problem* const p;
  ba_result* const r;
  StopCheck stop;
  LmScalars lm;
  Huber hb;
  int NP, NX, NE, nP, n;
  int n_blocks_e = 0, n_pairs = 0, n_tiles = 0, tile = kTileEdges;
  int cur = 0;
  int trials = 0;
  int robust;                          // Huber kernels on every edge: the value of the round that is running

  BaRun(ba_handle* h_, const ba_problem* p_, ba_result* r_, StopRef ref, int nP_, int robust_)
      : h(h_), st(h_->stream), p(p_), r(r_), NP(p_->n_poses), NX(p_->n_points), NE(p_->n_edges), nP(nP_), n(6 * nP_), robust(robust_ ? 1 : 0) {
    stop.ref = ref;
    hb.delta_mono = (float)std::sqrt(5.99); hb.dsqr_mono = hb.delta_mono * hb.delta_mono;           // S/Optimizer.cc:131-132: 5.99 here, not the local BA's 5.991
    hb.delta_stereo = (float)std::sqrt(7.815); hb.dsqr_stereo = hb.delta_stereo * hb.delta_stereo;
    n_blocks_e = (NE + 255) / 256;
  }

  void initial_state() {
    h->s_poses.resize((size_t)std::max(NP, 1));
    h->s_points.resize(3 * (size_t)std::max(NX, 1));
    h->s_pose_col.resize((size_t)std::max(NP, 1));
    int c = 0;
    for (int i = 0; i < NP; i++) {                                // Converter::toSE3Quat
      const float* T = p->poses + 16 * (size_t)i;
      const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
      PoseQ& q = h->s_poses[i];
      quat_from_R(R, q.q);
      quat_normalize(q.q);
      q.t[0] = T[3]; q.t[1] = T[7]; q.t[2] = T[11];
      h->s_pose_col[i] = p->pose_fixed[i] ? -1 : c++;
    }
    for (size_t i = 0; i < 3 * (size_t)NX; i++) h->s_points[i] = p->points[i];
  }

  // the estimate (host arrays) -> the caller's float32 result: Converter::toCvMat(SE3Quat), Converter::toCvMat(Vector3d)
  void write_state(const PoseQ* poses, const double* points) {
    for (int i = 0; i < NP; i++) {
      double R[9];
      quat_to_R(poses[i].q, R);
      float* T = r->poses + 16 * (size_t)i;
      for (int a = 0; a < 3; a++) { for (int c = 0; c < 3; c++) T[4 * a + c] = (float)R[3 * a + c]; T[4 * a + 3] = (float)poses[i].t[a]; }
      T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
    }
    for (size_t i = 0; i < 3 * (size_t)NX; i++) r->points[i] = (float)points[i];
  }
  void write_included() {
    if (!r->point_included) return;
    memset(r->point_included, 0, (size_t)NX);
    for (int k = 0; k < NE; k++) r->point_included[p->edges[k].point] = 1;
  }

  // optimize() never ran an iteration: the unchanged estimate goes back through the same conversions, no residual was computed
  int finish_without_iterations() {
    write_state(h->s_poses.data(), h->s_points.data());
    write_included();
    for (int k = 0; k < NE; k++) {
      if (r->edge_chi2) r->edge_chi2[k] = 0;
      if (r->edge_depth_pos) {
        const lba_edge& e = p->edges[k];
        double rr[3];
        quat_rotate(h->s_poses[e.pose].q, &h->s_points[3 * (size_t)e.point], rr);
        r->edge_depth_pos[k] = rr[2] + h->s_poses[e.pose].t[2] > 0.0 ? 1 : 0;
      }
    }
    return ORBG_OK;
  }

  int buffers() {
    int rc;
    const size_t sNP = (size_t)std::max(NP, 1), sNX = (size_t)std::max(NX, 1), sNE = (size_t)std::max(NE, 1), snP = (size_t)std::max(nP, 1);
    for (int b = 0; b < 2; b++)
      if ((rc = h->d_poses[b].reserve(sNP)) || (rc = h->d_points[b].reserve(3 * sNX))) return rc;
    if ((rc = h->d_edges.reserve(sNE)) || (rc = h->d_pose_col.reserve(sNP)) || (rc = h->d_pose_cam.reserve(sNP)) ||
        (rc = h->d_cams.reserve((size_t)std::max(p->n_cameras, 1))) || (rc = h->d_pt_start.reserve(sNX)) || (rc = h->d_pt_end.reserve(sNX)) ||
        (rc = h->d_chi2.reserve(sNE)) || (rc = h->d_partial.reserve((size_t)std::max(n_blocks_e, 1))) || (rc = h->d_EB.reserve(sNE * kEB)) ||
        (rc = h->d_Hll.reserve(6 * sNX)) || (rc = h->d_bl.reserve(3 * sNX)) || (rc = h->d_Hpp.reserve(21 * snP)) ||
        (rc = h->d_bp.reserve(6 * snP)) || (rc = h->d_Dinv.reserve(6 * sNX)) || (rc = h->d_Db.reserve(3 * sNX)) ||
        (rc = h->d_bs.reserve(6 * snP)) || (rc = h->d_x.reserve(6 * snP)) || (rc = h->d_scale_v.reserve(sNP + sNX)) ||
        (rc = h->d_depth.reserve(sNE)) || (rc = h->d_ok.reserve(4)) || (rc = h->d_rec.reserve(1)) || (rc = h->rec.reserve(1)) ||
        (rc = h->d_total.reserve(4)) || (rc = h->total_h.reserve(4)))
      return rc;
    return h->ldlt.plan(n, st);
  }

  int upload() {
    h->s_cams.resize((size_t)std::max(p->n_cameras, 1));
    for (int c = 0; c < p->n_cameras; c++) {
      const ba_camera& bc = p->cameras[c];
      CamRig g;
      g.c = Cam{bc.fx, bc.fy, bc.cx, bc.cy, bc.bf, bc.bf};
      g.has_right = 0;
      if (!cam_model_from(bc.model, &g.left)) return ORBG_BAD_ARG;
      g.right = g.left;
      g.Trl = PoseQ{{0, 0, 0, 1}, {0, 0, 0}};
      h->s_cams[c] = g;
    }
    // (pageable sources: hipMemcpyAsync returns once the bytes are staged, the host arrays may be reused afterwards)
    if (NP > 0) {
      ORBG_HIP(hipMemcpyAsync(h->d_poses[0].p, h->s_poses.data(), sizeof(PoseQ) * (size_t)NP, hipMemcpyHostToDevice, st));
      ORBG_HIP(hipMemcpyAsync(h->d_pose_col.p, h->s_pose_col.data(), sizeof(int) * (size_t)NP, hipMemcpyHostToDevice, st));
      ORBG_HIP(hipMemcpyAsync(h->d_pose_cam.p, p->pose_camera, sizeof(int) * (size_t)NP, hipMemcpyHostToDevice, st));
      ORBG_HIP(hipMemcpyAsync(h->d_cams.p, h->s_cams.data(), sizeof(CamRig) * (size_t)p->n_cameras, hipMemcpyHostToDevice, st));
    }
    if (NX > 0) ORBG_HIP(hipMemcpyAsync(h->d_points[0].p, h->s_points.data(), sizeof(double) * 3 * (size_t)NX, hipMemcpyHostToDevice, st));
    if (NE > 0) ORBG_HIP(hipMemcpyAsync(h->d_edges.p, p->edges, sizeof(lba_edge) * (size_t)NE, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipStreamSynchronize(st));
    return ORBG_OK;
  }

  int read_total(long long* out) {
    ORBG_HIP(hipMemcpyAsync(h->total_h.h, h->d_total.p, sizeof(long long), hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipStreamSynchronize(st));
    *out = h->total_h.h[0];
    return ORBG_OK;
  }

  // ---- BlockSolver::buildStructure on the device
  int structure() {
    int rc;
    h->timer.begin(kPhStructure, st);
    if (NX > 0) {
      ORBG_HIP(hipMemsetAsync(h->d_pt_start.p, 0, sizeof(int) * (size_t)NX, st));
      ORBG_HIP(hipMemsetAsync(h->d_pt_end.p, 0, sizeof(int) * (size_t)NX, st));
    }
    if (NE > 0) hipLaunchKernelGGL(k_ba_ranges, dim3(n_blocks_e), dim3(256), 0, st, NE, h->d_edges.p, h->d_pt_start.p, h->d_pt_end.p);
    if (nP == 0) { h->timer.end(st); ORBG_HIP(hipGetLastError()); return ORBG_OK; }
    // the edges of every free pose, ascending
    tile = kTileEdges * std::max(1, (int)(((long long)NE + (long long)kTileEdges * kMaxTiles - 1) / ((long long)kTileEdges * kMaxTiles)));
    n_tiles = std::max(1, (int)(((long long)NE + tile - 1) / tile));
    if ((rc = h->d_table.reserve((size_t)n_tiles * nP)) || (rc = h->d_row_count.reserve((size_t)nP)) || (rc = h->d_row_start.reserve((size_t)nP + 1)))
      return rc;
    hipLaunchKernelGGL(k_ba_tile_count, dim3(n_tiles), dim3(256), 0, st, NE, tile, h->d_edges.p, h->d_pose_col.p, nP, h->d_table.p);
    hipLaunchKernelGGL(k_ba_tile_scan, dim3((nP + 255) / 256), dim3(256), 0, st, n_tiles, nP, h->d_table.p, h->d_row_count.p);
    hipLaunchKernelGGL(k_ba_scan, dim3(1), dim3(1024), 0, st, nP, h->d_row_count.p, h->d_row_start.p, h->d_total.p);
    ORBG_HIP(hipGetLastError());
    long long n_free_edges = 0;
    if ((rc = read_total(&n_free_edges))) return rc;
    if (n_free_edges > NE) return ORBG_INTERNAL;
    if ((rc = h->d_row_edges.reserve((size_t)std::max<long long>(n_free_edges, 1)))) return rc;
    hipLaunchKernelGGL(k_ba_tile_place, dim3(n_tiles), dim3(256), 0, st, NE, tile, h->d_edges.p, h->d_pose_col.p, nP, h->d_table.p,
                       h->d_row_start.p, h->d_row_edges.p);
    // the non-empty pose pairs
    const int W = (nP + 31) / 32;
    if ((rc = h->d_bitmap.reserve((size_t)nP * W)) || (rc = h->d_pair_cnt.reserve((size_t)nP)) || (rc = h->d_pair_row_start.reserve((size_t)nP + 1)))
      return rc;
    ORBG_HIP(hipMemsetAsync(h->d_bitmap.p, 0, sizeof(unsigned) * (size_t)nP * W, st));
    if (NX > 0 && NE > 0)
      hipLaunchKernelGGL(k_ba_pair_mark, dim3((NX + 255) / 256), dim3(256), 0, st, NX, h->d_pt_start.p, h->d_pt_end.p, h->d_edges.p,
                         h->d_pose_col.p, W, h->d_bitmap.p);
    hipLaunchKernelGGL(k_ba_pair_count, dim3((nP + 255) / 256), dim3(256), 0, st, nP, W, h->d_bitmap.p, h->d_pair_cnt.p);
    hipLaunchKernelGGL(k_ba_scan, dim3(1), dim3(1024), 0, st, nP, h->d_pair_cnt.p, h->d_pair_row_start.p, h->d_total.p);
    ORBG_HIP(hipGetLastError());
    long long np64 = 0;
    if ((rc = read_total(&np64))) return rc;
    if (np64 < nP || np64 > (long long)nP * (nP + 1) / 2) return ORBG_INTERNAL;
    n_pairs = (int)np64;
    if ((rc = h->d_pair_i.reserve((size_t)n_pairs)) || (rc = h->d_pair_j.reserve((size_t)n_pairs)) || (rc = h->d_item_cnt.reserve((size_t)n_pairs)) ||
        (rc = h->d_item_start.reserve((size_t)n_pairs + 1)))
      return rc;
    hipLaunchKernelGGL(k_ba_pair_emit, dim3((nP + 255) / 256), dim3(256), 0, st, nP, W, h->d_bitmap.p, h->d_pair_row_start.p, h->d_pair_i.p,
                       h->d_pair_j.p);
    // their items
    hipLaunchKernelGGL(k_ba_items_count, dim3(n_pairs), dim3(256), 0, st, n_pairs, h->d_pair_i.p, h->d_pair_j.p, h->d_row_start.p,
                       h->d_row_edges.p, h->d_edges.p, h->d_pt_start.p, h->d_pt_end.p, h->d_pose_col.p, h->d_item_cnt.p);
    hipLaunchKernelGGL(k_ba_scan, dim3(1), dim3(1024), 0, st, n_pairs, h->d_item_cnt.p, h->d_item_start.p, h->d_total.p);
    ORBG_HIP(hipGetLastError());
    long long n_items = 0;
    if ((rc = read_total(&n_items))) return rc;
    if (n_items > 0x7FFFFFFFll) return ORBG_CAP_EXCEEDED;        // 32-bit offsets into the item list
    if ((rc = h->d_items.reserve((size_t)std::max<long long>(n_items, 1)))) return rc;
    hipLaunchKernelGGL(k_ba_items_fill, dim3(n_pairs), dim3(256), 0, st, n_pairs, h->d_pair_i.p, h->d_pair_j.p, h->d_row_start.p,
                       h->d_row_edges.p, h->d_edges.p, h->d_pt_start.p, h->d_pt_end.p, h->d_pose_col.p, h->d_item_start.p, h->d_items.p);
    h->timer.end(st);
    ORBG_HIP(hipGetLastError());
    return ORBG_OK;
  }

  // the record of the last launches, on the host
  int fetch_record() { return lm_fetch_record(h->rec.h, h->d_rec.p, st, h->timer); }

  // computeActiveErrors + buildSystem of state `buf`; the record brings chi2 and the largest diagonal entry
  int linearise(int buf) {
    h->timer.begin(kPhLin, st);
    if (NE > 0) {
      hipLaunchKernelGGL(k_ba_lin, dim3(n_blocks_e), dim3(256), 0, st, NE, h->d_edges.p, h->d_poses[buf].p, h->d_points[buf].p, h->d_pose_cam.p,
                         h->d_cams.p, robust, hb, h->d_chi2.p, h->d_partial.p, h->d_EB.p);
    }
    if (NX > 0)
      hipLaunchKernelGGL(k_schur_points<kEB>, dim3((NX + 255) / 256), dim3(256), 0, st, NX, h->d_pt_start.p, h->d_pt_end.p, h->d_EB.p, h->d_Hll.p, h->d_bl.p);
    if (nP > 0)
      hipLaunchKernelGGL(k_ba_poses, dim3(nP), dim3(256), 0, st, h->d_row_start.p, h->d_row_edges.p, h->d_edges.p, h->d_poses[buf].p,
                         h->d_points[buf].p, h->d_pose_cam.p, h->d_cams.p, robust, hb, h->d_chi2.p, h->d_Hpp.p, h->d_bp.p);
    hipLaunchKernelGGL(k_ba_finish, dim3(1), dim3(256), 0, st, n_blocks_e, h->d_partial.p, 0, h->d_scale_v.p, nP, h->d_Hpp.p, NX, h->d_Hll.p,
                       h->d_pt_start.p, h->d_pt_end.p, (const int*)nullptr, h->d_rec.p);
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
    if (nP > 0) {
      if ((rc = h->ldlt.clear(h->d_x.p, st))) return rc;
      hipLaunchKernelGGL(k_ba_schur, dim3(n_pairs), dim3(256), 0, st, nP, h->d_pair_i.p, h->d_pair_j.p, h->d_item_start.p, h->d_items.p,
                         h->d_edges.p, h->d_EB.p, h->d_Dinv.p, h->d_Db.p, h->d_Hpp.p, h->d_bp.p, lambda, h->ldlt.S(), h->d_bs.p,
                         h->ldlt.St());
    }
    h->timer.end(st);
    h->timer.begin(kPhLdlt, st);
    if (nP > 0) {
      if ((rc = h->ldlt.launch(h->d_bs.p, h->d_x.p, h->d_ok.p, st))) return rc;
    } else {
      hipLaunchKernelGGL(k_ba_set_ok, dim3(1), dim3(1), 0, st, h->d_ok.p);
    }
    h->timer.end(st);
    h->timer.begin(kPhUpdate, st);
    hipLaunchKernelGGL(k_ba_update, dim3((NP + NX + 255) / 256), dim3(256), 0, st, NP, NX, h->d_pose_col.p, h->d_poses[from].p, h->d_points[from].p,
                       h->d_x.p, h->d_pt_start.p, h->d_pt_end.p, h->d_edges.p, h->d_EB.p, h->d_Dinv.p, h->d_bl.p, h->d_bp.p, lambda, h->d_ok.p,
                       h->d_poses[to].p, h->d_points[to].p, h->d_scale_v.p);
    if (NE > 0)
      hipLaunchKernelGGL(k_ba_errors, dim3(n_blocks_e), dim3(256), 0, st, NE, h->d_edges.p, h->d_poses[to].p, h->d_points[to].p, h->d_pose_cam.p,
                         h->d_cams.p, robust, hb, h->d_chi2.p, h->d_partial.p);
    hipLaunchKernelGGL(k_ba_finish, dim3(1), dim3(256), 0, st, n_blocks_e, h->d_partial.p, NP + NX, h->d_scale_v.p, 0, (const double*)nullptr, 0,
                       (const double*)nullptr, h->d_pt_start.p, h->d_pt_end.p, h->d_ok.p, h->d_rec.p);
    h->timer.end(st);
    trials++;
    return fetch_record();
  }

  // ---- what lm_optimize (lm_driver.hpp) asks of a solve
  int linearise() { return linearise(cur); }
  const LmRec& record() const { return *h->rec.h; }
  int timed_out() const { return ldlt_timed_out_rc(h->rec.h->ok); }
  void accept() { cur ^= 1; }
  int first_linearisation(double* user_lambda) {
    *user_lambda = 0.0;
    r->chi2_initial = lm.currentChi;
    return ORBG_OK;
  }
  void iteration_done(int qmax, bool) {
    r->chi2_final = lm.currentChi;
    lm_trace_row(lm, qmax, r->trace, r->trace_cap, &r->trace_len);
  }
  int optimize(int iterations, int* done) { return lm_optimize(*this, iterations, stop, done); }

  // ---- results: chi2 of the LAST error evaluation, depth test with the final estimate
  int download() {
    if (NE > 0 && r->edge_depth_pos) {
      hipLaunchKernelGGL(k_ba_depth, dim3(n_blocks_e), dim3(256), 0, st, NE, h->d_edges.p, h->d_poses[cur].p, h->d_points[cur].p, h->d_depth.p);
      ORBG_HIP(hipGetLastError());
      ORBG_HIP(hipMemcpyAsync(r->edge_depth_pos, h->d_depth.p, (size_t)NE, hipMemcpyDeviceToHost, st));
    }
    if (NE > 0 && r->edge_chi2) ORBG_HIP(hipMemcpyAsync(r->edge_chi2, h->d_chi2.p, sizeof(double) * (size_t)NE, hipMemcpyDeviceToHost, st));
    if (NP > 0) ORBG_HIP(hipMemcpyAsync(h->s_poses.data(), h->d_poses[cur].p, sizeof(PoseQ) * (size_t)NP, hipMemcpyDeviceToHost, st));
    if (NX > 0) ORBG_HIP(hipMemcpyAsync(h->s_points.data(), h->d_points[cur].p, sizeof(double) * 3 * (size_t)NX, hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipStreamSynchronize(st));
    write_state(h->s_poses.data(), h->s_points.data());
    write_included();
    return ORBG_OK;
  }
};

// optimize(n) with n <= 0, nothing to optimise, or the flag already up: g2o runs no iteration, and the solve needs no device
bool ba_runs_no_iteration(const ba_problem* p, StopRef ref) {
  StopCheck stop;
  stop.ref = ref;
  stop.past_precheck = true;
  return p->iterations <= 0 || p->n_edges == 0 || stop();
}

int ba_attempt(ba_handle* h, const ba_problem* p, StopRef ref, ba_result* r, int nP) {
  BaRun run(h, p, r, ref, nP, p->robust);
  int rc;
  r->status = LBA_APPLIED; r->iters = 0; r->trace_len = 0; r->chi2_initial = r->chi2_final = 0;
  if (run.stop()) r->status = LBA_ABORTED_BEFORE_OPT;
  run.stop.past_precheck = true;
  run.initial_state();
  if (ba_runs_no_iteration(p, ref)) return run.finish_without_iterations();       // (uses the handle's host arrays only)
  if ((rc = select_device(h->device))) return rc;
  if ((rc = h->timer.reset())) return rc;
  StreamDrain drain{h->stream};
  if ((rc = run.buffers()) || (rc = run.upload()) || (rc = run.structure())) return rc;
  int done = 0;
  if ((rc = run.optimize(p->iterations, &done))) return rc;
  r->iters = done;
  if (done == 0) return run.finish_without_iterations();
  rc = run.download();
  h->timer.flush(h->stream);
  return rc;
}

int ba_solve_impl(ba_handle* h, const ba_problem* p, StopRef ref, ba_result* r, int validated_free = -1) {
  if (!h) return ORBG_BAD_ARG;
  int nP = validated_free, rc;
  if (nP < 0 && (rc = ba_validate(p, r, &nP))) return rc;
  // (a timed-out launch: solved again on the one-workgroup kernels, which this handle then keeps using)
  return ldlt_retry(h->ldlt, h->stream, [&] { return ba_attempt(h, p, ref, r, nP); });
}

int ba_solve_once(const ba_problem* p, StopRef ref, ba_result* r) {
  int nP = 0;
  int rc = ba_validate(p, r, &nP);               // refusals come before a handle (a stream) exists
  if (rc) return rc;
  if (ba_runs_no_iteration(p, ref)) {
    ba_handle host;                              // host arrays only: no device is selected, no stream created
    return ba_attempt(&host, p, ref, r, nP);
  }
  ba_handle* h = nullptr;
  if ((rc = ba_create(p->device, p->n_poses, p->n_points, p->n_edges, &h))) return rc;
  rc = ba_solve_impl(h, p, ref, r, nP);
  ba_destroy(h);
  return rc;
}

// ---------------------------------------------------------------------------------------------- welding BA

int weld_validate(const ba_weld_problem* wp, const ba_weld_result* wr, int* n_free) {
  if (!wp || !wr) return ORBG_BAD_ARG;
  if (wp->struct_size < sizeof(ba_weld_problem) || wr->struct_size < sizeof(ba_weld_result)) return ORBG_BAD_ARG;
  if (!std::isfinite(wp->chi2_mono) || !std::isfinite(wp->chi2_stereo) || !(wp->chi2_mono > 0) || !(wp->chi2_stereo > 0)) return ORBG_BAD_ARG;
  if (wr->trace_second && wr->trace_second_cap < 0) return ORBG_BAD_ARG;
  const int rc = ba_validate(&wp->ba, &wr->ba, n_free);
  if (rc) return rc;
  if (!wr->edge_level && wp->ba.n_edges > 0) return ORBG_BAD_ARG;
  return ORBG_OK;
}

template <class T>
void exchange(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

// While round 2 runs, the run's edge list, its count and the per-edge chi2 are those of the level-0 edges, and the trace it writes
// is the second one: the handle's buffers and the result's round fields are exchanged here and put back on every way out.
struct WeldSecondRound {
  BaRun& run;
  ba_weld_result* const wr;
  const int NE_all, blocks_all, robust_first;
  const ba_result first;
  WeldSecondRound(BaRun& run_, ba_weld_result* wr_, int n_kept)
      : run(run_), wr(wr_), NE_all(run_.NE), blocks_all(run_.n_blocks_e), robust_first(run_.robust), first(*run_.r) {
    exchange(run.h->d_edges, run.h->d_edges_kept);
    exchange(run.h->d_chi2, run.h->d_chi2_kept);
    run.NE = n_kept; run.n_blocks_e = (n_kept + 255) / 256; run.robust = 0;
    ba_result* r = run.r;
    r->trace = wr->trace_second; r->trace_cap = wr->trace_second ? wr->trace_second_cap : 0; r->trace_len = 0;
    r->chi2_initial = r->chi2_final = 0;
  }
  ~WeldSecondRound() {
    ba_result* r = run.r;
    wr->chi2_initial_second = r->chi2_initial; wr->chi2_final_second = r->chi2_final; wr->trace_second_len = r->trace_len;
    r->trace = first.trace; r->trace_cap = first.trace_cap; r->trace_len = first.trace_len;
    r->chi2_initial = first.chi2_initial; r->chi2_final = first.chi2_final;
    run.NE = NE_all; run.n_blocks_e = blocks_all; run.robust = robust_first;
    exchange(run.h->d_edges, run.h->d_edges_kept);
    exchange(run.h->d_chi2, run.h->d_chi2_kept);
  }
};

int weld_attempt(ba_handle* h, const ba_weld_problem* wp, StopRef ref, ba_weld_result* wr, int nP) {
  const ba_problem* p = &wp->ba;
  ba_result* r = &wr->ba;
  BaRun run(h, p, r, ref, nP, 1);                  // round 1: Huber kernels on every edge, whatever p->robust says
  int rc;
  r->status = LBA_APPLIED; r->iters = 0; r->trace_len = 0; r->chi2_initial = r->chi2_final = 0;
  wr->n_level1 = 0; wr->rounds_run = 0; wr->iters_second = 0; wr->trace_second_len = 0;
  wr->chi2_initial_second = wr->chi2_final_second = 0;
  if (p->n_edges > 0) memset(wr->edge_level, 0, (size_t)p->n_edges);
  if (run.stop()) r->status = LBA_ABORTED_BEFORE_OPT;
  run.stop.past_precheck = true;
  run.initial_state();
  if (ba_runs_no_iteration(p, ref)) return run.finish_without_iterations();       // (uses the handle's host arrays only)
  if ((rc = select_device(h->device))) return rc;
  if ((rc = h->timer.reset())) return rc;
  StreamDrain drain{h->stream};
  if ((rc = run.buffers()) || (rc = run.upload()) || (rc = run.structure())) return rc;
  int done = 0;
  if ((rc = run.optimize(p->iterations, &done))) return rc;
  r->iters = done;
  if (done == 0) return run.finish_without_iterations();
  wr->rounds_run = 1;
  const int NE = run.NE;
  if (!run.stop()) {                               // S/Optimizer.cc:6606: bDoMore
    const size_t sNE = (size_t)NE;
    if ((rc = h->d_level.reserve(sNE)) || (rc = h->d_keep.reserve(sNE)) || (rc = h->d_keep_off.reserve(sNE + 1)) ||
        (rc = h->d_origin.reserve(sNE)) || (rc = h->d_edges_kept.reserve(sNE)) || (rc = h->d_chi2_kept.reserve(sNE)))
      return rc;
    h->timer.begin(kPhStructure, run.st);
    hipLaunchKernelGGL(k_ba_weld_classify, dim3(run.n_blocks_e), dim3(256), 0, run.st, NE, h->d_edges.p, h->d_poses[run.cur].p,
                       h->d_points[run.cur].p, h->d_chi2.p, wp->chi2_mono, wp->chi2_stereo, h->d_level.p, h->d_keep.p);
    hipLaunchKernelGGL(k_ba_scan, dim3(1), dim3(1024), 0, run.st, NE, h->d_keep.p, h->d_keep_off.p, h->d_total.p);
    hipLaunchKernelGGL(k_ba_weld_compact, dim3(run.n_blocks_e), dim3(256), 0, run.st, NE, h->d_edges.p, h->d_keep.p, h->d_keep_off.p,
                       h->d_edges_kept.p, h->d_origin.p);
    h->timer.end(run.st);
    ORBG_HIP(hipGetLastError());
    ORBG_HIP(hipMemcpyAsync(wr->edge_level, h->d_level.p, sNE, hipMemcpyDeviceToHost, run.st));
    long long kept64 = 0;
    if ((rc = run.read_total(&kept64))) return rc;
    if (kept64 < 0 || kept64 > NE) return ORBG_INTERNAL;
    const int n_kept = (int)kept64;
    wr->n_level1 = NE - n_kept;
    if (n_kept > 0 && wp->iterations_second > 0) {
      int done2 = 0;
      {
        WeldSecondRound second(run, wr, n_kept);
        wr->rounds_run = 2;
        if (!(rc = run.structure())) rc = run.optimize(wp->iterations_second, &done2);
      }
      if (rc) return rc;
      wr->iters_second = done2;
      if (done2 > 0) {
        hipLaunchKernelGGL(k_ba_weld_scatter, dim3((n_kept + 255) / 256), dim3(256), 0, run.st, n_kept, h->d_origin.p, h->d_chi2_kept.p,
                           h->d_chi2.p);
        ORBG_HIP(hipGetLastError());
      }
    }
  }
  rc = run.download();
  h->timer.flush(h->stream);
  return rc;
}

int weld_solve_impl(ba_handle* h, const ba_weld_problem* wp, StopRef ref, ba_weld_result* wr, int validated_free = -1) {
  if (!h) return ORBG_BAD_ARG;
  int nP = validated_free, rc;
  if (nP < 0 && (rc = weld_validate(wp, wr, &nP))) return rc;
  // (as in ba_solve_impl, for the whole call: both rounds again)
  return ldlt_retry(h->ldlt, h->stream, [&] { return weld_attempt(h, wp, ref, wr, nP); });
}

int weld_solve_once(const ba_weld_problem* wp, StopRef ref, ba_weld_result* wr) {
  int nP = 0;
  int rc = weld_validate(wp, wr, &nP);
  if (rc) return rc;
  if (ba_runs_no_iteration(&wp->ba, ref)) {
    ba_handle host;
    return weld_attempt(&host, wp, ref, wr, nP);
  }
  ba_handle* h = nullptr;
  if ((rc = ba_create(wp->ba.device, wp->ba.n_poses, wp->ba.n_points, wp->ba.n_edges, &h))) return rc;
  rc = weld_solve_impl(h, wp, ref, wr, nP);
  ba_destroy(h);
  return rc;
}

}  // namespace

extern "C" int ba_create(int device, int cap_poses, int cap_points, int cap_edges, ba_handle** out) {
  if (!out || cap_poses < 0 || cap_points < 0 || cap_edges < 0) return ORBG_BAD_ARG;
  int rc = select_device(device);
  if (rc) return rc;
  ba_handle* h = new ba_handle();
  h->device = device;
  h->ldlt.read_env();
  if (orbg::create_stream(&h->stream, "lba") != hipSuccess) { delete h; return ORBG_HIP_ERROR; }
  (void)cap_poses; (void)cap_points; (void)cap_edges;   // unused: buffers grow on first use and are kept
  *out = h;
  return ORBG_OK;
}

extern "C" int ba_destroy(ba_handle* h) {
  if (!h) return ORBG_BAD_ARG;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->ldlt.release();
  h->d_edges.release();
  for (int i = 0; i < 2; i++) { h->d_poses[i].release(); h->d_points[i].release(); }
  for (DevBuf<int>* b : {&h->d_pose_col, &h->d_pose_cam, &h->d_pt_start, &h->d_pt_end, &h->d_table, &h->d_row_count, &h->d_row_start, &h->d_row_edges,
                         &h->d_pair_cnt, &h->d_pair_row_start, &h->d_pair_i, &h->d_pair_j, &h->d_item_cnt, &h->d_item_start, &h->d_ok})
    b->release();
  for (DevBuf<double>* b : {&h->d_chi2, &h->d_partial, &h->d_EB, &h->d_Hll, &h->d_bl, &h->d_Hpp, &h->d_bp, &h->d_Dinv, &h->d_Db, &h->d_bs,
                            &h->d_x, &h->d_scale_v})
    b->release();
  h->d_edges_kept.release(); h->d_chi2_kept.release(); h->d_level.release(); h->d_keep.release(); h->d_keep_off.release(); h->d_origin.release();
  h->d_bitmap.release(); h->d_total.release(); h->d_items.release(); h->d_cams.release(); h->d_depth.release(); h->d_rec.release();
  h->rec.release(); h->total_h.release();
  h->timer.release();
  orbg::release_stream(h->stream);
  delete h;
  return ORBG_OK;
}

extern "C" int ba_solve_h(ba_handle* h, const ba_problem* p, const volatile int32_t* stop_flag, ba_result* r) {
  StopRef s; s.i32 = stop_flag;
  return ba_solve_impl(h, p, s, r);
}
extern "C" int ba_solve_hb(ba_handle* h, const ba_problem* p, const volatile uint8_t* stop_bool, ba_result* r) {
  StopRef s; s.u8 = stop_bool;
  return ba_solve_impl(h, p, s, r);
}
extern "C" int ba_solve(const ba_problem* p, const volatile int32_t* stop_flag, ba_result* r) {
  StopRef s; s.i32 = stop_flag;
  return ba_solve_once(p, s, r);
}
extern "C" int ba_solve_b(const ba_problem* p, const volatile uint8_t* stop_bool, ba_result* r) {
  StopRef s; s.u8 = stop_bool;
  return ba_solve_once(p, s, r);
}
extern "C" int ba_weld_solve_h(ba_handle* h, const ba_weld_problem* p, const volatile int32_t* stop_flag, ba_weld_result* r) {
  StopRef s; s.i32 = stop_flag;
  return weld_solve_impl(h, p, s, r);
}
extern "C" int ba_weld_solve_hb(ba_handle* h, const ba_weld_problem* p, const volatile uint8_t* stop_bool, ba_weld_result* r) {
  StopRef s; s.u8 = stop_bool;
  return weld_solve_impl(h, p, s, r);
}
extern "C" int ba_weld_solve(const ba_weld_problem* p, const volatile int32_t* stop_flag, ba_weld_result* r) {
  StopRef s; s.i32 = stop_flag;
  return weld_solve_once(p, s, r);
}
extern "C" int ba_weld_solve_b(const ba_weld_problem* p, const volatile uint8_t* stop_bool, ba_weld_result* r) {
  StopRef s; s.u8 = stop_bool;
  return weld_solve_once(p, s, r);
}
extern "C" int ba_set_profiling(ba_handle* h, int on) {
  if (!h) return ORBG_BAD_ARG;
  h->timer.on = on != 0;
  return ORBG_OK;
}
extern "C" int ba_get_phase_ms(ba_handle* h, double* ms) {
  if (!h || !ms) return ORBG_BAD_ARG;
  for (int i = 0; i < 5; i++) ms[i] = h->timer.ms[i];
  return ORBG_OK;
}
