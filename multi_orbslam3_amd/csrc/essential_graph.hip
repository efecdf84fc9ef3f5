// liborbgpu -- the Sim3 pose graph of loop closing for gfx950 (MI355X).  Replaces the numerical core of
// Optimizer::OptimizeEssentialGraph (S/Optimizer.cc:2413-2747, called by LoopClosing::CorrectLoop at S/LoopClosing.cc:1272; the forms
// at S/Optimizer.cc:3196 and :3596 build the same problem) behind eg_solve() of include/orbgpu.h: g2o::VertexSim3Expmap vertices,
// g2o::EdgeSim3 edges with identity information and no robust kernel, setUserLambdaInit, ONE optimize(iterations), then the map
// points through the initial and the final estimate of their reference keyframe.
//
// The Sim3 arithmetic is sim3_math.hpp's, the LM decisions lm_step.hpp's and their outer loop lm_driver.hpp's, the LDL^T solvers the bundle adjustments'
// (ldlt_mfma.hpp, ldlt_xcd.hpp, ldlt_wide.hpp), chosen by n = 7 F as full_ba.hip chooses by 6 nP.  There is no Schur complement: every
// vertex is a pose, the normal equations H (7F x 7F, F free vertices in ascending vertex order) go to the solver dense.
//   structure, once per call, on the host (thousands of edges): per free vertex its (edge, side) items in edge order, the distinct
//     free-free vertex pairs in order of first appearance with their (edge, orientation) items in edge order
//   per LM iteration:
//     k_eg_lin     32 lanes per edge: lane 0 the error log(C Siw Sjw^-1), lanes 1 .. 28 the error at Sim3(+-delta e_d) * estimate of
//                  vertex i / vertex j (G/core/base_binary_edge.hpp:131-205, delta = 1e-9, through oplusImpl, which zeroes update[6]
//                  under _fix_scale: both evaluations of that column meet the same estimate, the column is exactly 0); then the
//                  lanes of the edge form Ji, Jj = scalar * (e+ - e-) and store them with e.  A fixed vertex gets no Jacobian.
//     k_eg_blocks  one wavefront per free vertex / per pair: the 7 x 7 block as the sum over its items, in item order, of Jx^T Jy
//                  (information = I, G/core/base_binary_edge.hpp:74-90), and b = sum Jx^T (-e)
//   per trial:
//     one fill of the dense system, k_eg_scatter writes the blocks with lambda on the diagonal, LDL^T by size, k_eg_update
//     (oplus per vertex, computeScale terms), k_eg_errors (chi2 of the trial state), k_eg_finish -> the record the host reads
//   after the last iteration, in the same submission: k_eg_points, one thread per map point.
// Every sum has a fixed order and there is no floating-point atomic: two calls on the same input return the same bits.

#include <unistd.h>

#include <atomic>

#include "common.hpp"
#include "wave.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <map>
#include <type_traits>
#include <vector>

#include "se3.hpp"
#include "sim3_math.hpp"
#include "lm_driver.hpp"
#include "lm_record.hpp"

using namespace orbg;
using namespace orbg_s3;
using namespace orbg_lm;

namespace {

#include "ldlt_mfma.hpp"
#include "ldlt_xcd.hpp"
#include "ldlt_wide.hpp"
#include "ldlt_solver.hpp"

constexpr int kEJ = 105;                 // per edge: Ji (7 x 7 row-major: error row, update column) | Jj | e
constexpr int kLinEdges = 8;             // edges per workgroup of k_eg_lin (32 lanes each)

struct EgEdge { int vi, vj; S3 C; };

// EdgeSim3::computeError, G/types/types_seven_dof_expmap.h:106-114: (C * v1) * v2^-1, then log()
__host__ __device__ inline void eg_error(const S3& C, const S3& Si, const S3& Sj, double* e) {
  S3 inv, a, b;
  s3_inverse(Sj, &inv);
  s3_mul(C, Si, &a);
  s3_mul(a, inv, &b);
  s3_log(b, e);
}

// VertexSim3Expmap::oplusImpl, G/types/types_seven_dof_expmap.h:60-69
__device__ inline void eg_oplus(const S3& est, double* u, bool fix_scale, S3* out) {
  if (fix_scale) u[6] = 0;
  S3 ex;
  s3_exp(u, &ex);
  s3_mul(ex, est, out);
}

__global__ __launch_bounds__(256) void k_eg_lin(int NE, const EgEdge* __restrict__ edges, const S3* __restrict__ est,
                                                const int* __restrict__ col, const int* __restrict__ fixs, double* __restrict__ EJ,
                                                double* __restrict__ partial) {
  __shared__ double se[kLinEdges][29][7];
  __shared__ double red[4];
  const int le = threadIdx.x >> 5, slot = threadIdx.x & 31;
  const int k = blockIdx.x * kLinEdges + le;
  int ci = -1, cj = -1;
  if (k < NE) {
    const EgEdge e = edges[k];
    ci = col[e.vi]; cj = col[e.vj];
    if (slot < 29) {
      S3 Si = est[e.vi], Sj = est[e.vj];
      bool need = true;
      if (slot >= 1) {
        const int side = slot >= 15 ? 1 : 0;
        const int q = slot - 1 - 14 * side, d = q >> 1;
        const double step = (q & 1) ? -1e-9 : 1e-9;        // errorBak = e(+delta); errorBak -= e(-delta)
        need = (side ? cj : ci) >= 0;
        if (need) {
          double u[7];
#pragma unroll
          for (int a = 0; a < 7; a++) u[a] = a == d ? step : 0.0;
          S3 pe;
          if (side) { eg_oplus(Sj, u, fixs[e.vj] != 0, &pe); Sj = pe; }
          else { eg_oplus(Si, u, fixs[e.vi] != 0, &pe); Si = pe; }
        }
      }
      if (need) {
        double r[7];
        eg_error(e.C, Si, Sj, r);
#pragma unroll
        for (int a = 0; a < 7; a++) se[le][slot][a] = r[a];
      }
    }
  }
  __syncthreads();
  double chi = 0;
  if (k < NE) {
    const double scalar = 1.0 / (2 * 1e-9);
    double* out = EJ + (size_t)k * kEJ;
    for (int idx = slot; idx < kEJ; idx += 32) {
      double v;
      if (idx < 98) {
        const int side = idx >= 49 ? 1 : 0, w = idx - 49 * side, r = w / 7, d = w % 7;
        const bool free_v = (side ? cj : ci) >= 0;
        v = free_v ? scalar * (se[le][1 + 14 * side + 2 * d][r] - se[le][2 + 14 * side + 2 * d][r]) : 0.0;
      } else {
        v = se[le][0][idx - 98];
      }
      out[idx] = v;
    }
    if (slot == 0)
      for (int a = 0; a < 7; a++) chi += se[le][0][a] * se[le][0][a];
  }
  const double s = block_sum_256(chi, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// chi2 = e^T e of every edge at state `est`, the workgroup's partial; optionally the error vectors
__global__ __launch_bounds__(256) void k_eg_errors(int NE, const EgEdge* __restrict__ edges, const S3* __restrict__ est,
                                                   double* __restrict__ partial, double* __restrict__ err_out) {
  __shared__ double red[4];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double chi = 0;
  if (k < NE) {
    const EgEdge e = edges[k];
    double r[7];
    eg_error(e.C, est[e.vi], est[e.vj], r);
#pragma unroll
    for (int a = 0; a < 7; a++) chi += r[a] * r[a];
    if (err_out) {
#pragma unroll
      for (int a = 0; a < 7; a++) err_out[7 * (size_t)k + a] = r[a];
    }
  }
  const double s = block_sum_256(chi, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// task t < F: Hd_t = sum Jx^T Jx, b_t = sum Jx^T (-e) over the items (edge << 1 | side) of free vertex t;
// task F + p: Hp_p = sum Jrow^T Jcol over the items (edge << 1 | flipped) of pair p (flipped: vertex j of the edge is the pair's row)
__global__ __launch_bounds__(64) void k_eg_blocks(int F, const int* __restrict__ task_start, const int* __restrict__ items,
                                                  const double* __restrict__ EJ, double* __restrict__ Hd, double* __restrict__ bv,
                                                  double* __restrict__ Hp) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const int b = task_start[t], e = task_start[t + 1];
  const bool diag = t < F;
  if (tid >= (diag ? 56 : 49)) return;
  const int a = tid < 49 ? tid / 7 : tid - 49, c = tid % 7;
  double acc = 0;
  for (int q = b; q < e; q++) {
    const int it = items[q];
    const double* J = EJ + (size_t)(it >> 1) * kEJ;
    const int f = it & 1;
    const double* Jr = J + 49 * f;                         // the block's row vertex
    const double* Jc = diag ? Jr : J + 49 * (f ^ 1);
    double h = 0;
    if (tid < 49) {
#pragma unroll
      for (int r = 0; r < 7; r++) h += Jr[7 * r + a] * Jc[7 * r + c];
    } else {
#pragma unroll
      for (int r = 0; r < 7; r++) h += Jr[7 * r + a] * (-J[98 + r]);
    }
    acc += h;
  }
  if (tid >= 49) bv[7 * (size_t)t + a] = acc;
  else if (diag) Hd[49 * (size_t)t + tid] = acc;
  else Hp[49 * (size_t)(t - F) + tid] = acc;
}

// the blocks into the dense system (row-major S, both triangles) or the matrix-core solvers' tile image, lambda on the diagonal
__global__ __launch_bounds__(64) void k_eg_scatter(int F, const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                   const double* __restrict__ Hd, const double* __restrict__ bv,
                                                   const double* __restrict__ Hp, double lambda, double* __restrict__ S,
                                                   double* __restrict__ St) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const bool diag = t < F;
  const int n = 7 * F;
  if (tid >= (diag ? 56 : 49)) return;
  if (tid >= 49) {
    if (St) ldltm::image_put_rhs(St, n, 7 * t + tid - 49, bv[7 * (size_t)t + tid - 49]);
    return;
  }
  const int a = tid / 7, c = tid % 7;
  const int bi = diag ? t : pair_i[t - F], bj = diag ? t : pair_j[t - F];
  double v = diag ? Hd[49 * (size_t)t + tid] : Hp[49 * (size_t)(t - F) + tid];
  if (diag && a == c) v += lambda;
  const int r = 7 * bi + a, cc = 7 * bj + c;
  if (St) {
    const int p0 = ldltm::tile_image_pos(r, cc);
    if (p0 >= 0) St[p0] = v;
    if (!diag) { const int p1 = ldltm::tile_image_pos(cc, r); if (p1 >= 0) St[p1] = v; }
  } else {
    S[(size_t)r * n + cc] = v;
    if (!diag) S[(size_t)cc * n + r] = v;
  }
}

// trial state = oplus(current, x) per vertex; its term of computeScale: sum_j x_j (lambda x_j + b_j)
__global__ __launch_bounds__(256) void k_eg_update(int NV, const int* __restrict__ col, const int* __restrict__ fixs, const S3* __restrict__ est,
                                                   const double* __restrict__ x, const double* __restrict__ bv, double lambda,
                                                   const int* __restrict__ ok_flag, S3* __restrict__ est_out, double* __restrict__ scale_v) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= NV) return;
  const int c = col[v];
  double sc = 0;
  if (c < 0 || *ok_flag == 0) est_out[v] = est[v];        // a failed solve leaves no step: the trial state is the current one
  else {
    double u[7];
#pragma unroll
    for (int a = 0; a < 7; a++) { u[a] = x[7 * c + a]; sc += u[a] * (lambda * u[a] + bv[7 * (size_t)c + a]); }
    S3 o;
    eg_oplus(est[v], u, fixs[v] != 0, &o);
    est_out[v] = o;
  }
  scale_v[v] = sc;
}

// one workgroup: the largest diagonal entry of a linearisation (Hd given), then lm_finish_record
__global__ __launch_bounds__(256) void k_eg_finish(int n_partial, const double* __restrict__ partial, int n_scale, const double* __restrict__ scale_v,
                                                   int F, const double* __restrict__ Hd, const int* __restrict__ ok_flag, LmRec* __restrict__ rec) {
  const int tid = threadIdx.x;
  double m = 0;
  if (Hd)
    for (int i = tid; i < 7 * F; i += 256) m = fmax(m, fabs(Hd[49 * (size_t)(i / 7) + 8 * (i % 7)]));
  lm_finish_record(n_partial, partial, n_scale, scale_v, m, ok_flag, rec);
}

// S/Optimizer.cc:2710-2743: correctedSwr.map(Srw.map(P)), Srw the vertex's INITIAL estimate, correctedSwr the inverse of its final one
__global__ __launch_bounds__(256) void k_eg_points(int NP, const eg_point* __restrict__ pts, const S3* __restrict__ est0,
                                                   const S3* __restrict__ est, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= NP) return;
  const eg_point p = pts[i];
  if (p.ref < 0) { out[3 * (size_t)i] = p.pos[0]; out[3 * (size_t)i + 1] = p.pos[1]; out[3 * (size_t)i + 2] = p.pos[2]; return; }
  S3 inv;
  s3_inverse(est[p.ref], &inv);
  const double P[3] = {(double)p.pos[0], (double)p.pos[1], (double)p.pos[2]};
  double a[3], b[3];
  s3_map(est0[p.ref], P, a);
  s3_map(inv, a, b);
  out[3 * (size_t)i] = (float)b[0]; out[3 * (size_t)i + 1] = (float)b[1]; out[3 * (size_t)i + 2] = (float)b[2];
}

// ---------------------------------------------------------------------------------------------- the calling thread's work area

struct EgBufs {
  LdltSolver ldlt;                     // the solver of the normal equations (its switches: read on the thread's first solve)
  DevBuf<EgEdge> d_edges;
  DevBuf<S3> d_est[3];                 // two LM states and the initial estimate
  DevBuf<int> d_col, d_fixs, d_task_start, d_items, d_pair_i, d_pair_j, d_ok;
  DevBuf<double> d_EJ, d_partial, d_Hd, d_bv, d_Hp, d_x, d_scale_v, d_err0;
  DevBuf<eg_point> d_pts;
  DevBuf<float> d_pts_out;
  DevBuf<LmRec> d_rec;
  PinnedBuf<LmRec> rec;
  PhaseTimer<4> timer;
  void release_buffers() {
    ldlt.release();
    d_edges.release();
    for (DevBuf<S3>& b : d_est) b.release();
    for (DevBuf<int>* b : {&d_col, &d_fixs, &d_task_start, &d_items, &d_pair_i, &d_pair_j, &d_ok}) b->release();
    for (DevBuf<double>* b : {&d_EJ, &d_partial, &d_Hd, &d_bv, &d_Hp, &d_x, &d_scale_v, &d_err0}) b->release();
    d_pts.release(); d_pts_out.release(); d_rec.release(); rec.release();
    timer.release();
  }
};
typedef WorkArea<EgBufs> EgArea;

std::atomic<int> g_eg_profiling{0};
thread_local double t_eg_phase_ms[4] = {0, 0, 0, 0};

enum { kPhLin = 0, kPhAssemble = 1, kPhLdlt = 2, kPhUpdate = 3 };

inline bool eg_finite(const double* v, int n) {
  for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
  return true;
}

// What can be refused is refused here, before a device is looked for.
int eg_validate(const eg_problem* p, const eg_result* r, int* n_free) {
  if (!p || !r) return ORBG_BAD_ARG;
  if (p->struct_size < sizeof(eg_problem) || r->struct_size < sizeof(eg_result)) return ORBG_BAD_ARG;
  if (p->n_vertices < 0 || p->n_edges < 0 || p->n_points < 0) return ORBG_BAD_ARG;
  if ((p->n_vertices > 0 && (!p->vertices || !r->estimates)) || (p->n_edges > 0 && !p->edges) || (p->n_points > 0 && (!p->points || !r->points)))
    return ORBG_BAD_ARG;
  if (!std::isfinite(p->lambda_init)) return ORBG_BAD_ARG;
  if (r->trace_cap < 0 || (r->trace_cap > 0 && !r->trace)) return ORBG_BAD_ARG;
  int F = 0;
  for (int i = 0; i < p->n_vertices; i++) {
    const eg_vertex& v = p->vertices[i];
    if (!eg_finite(v.q, 4) || !eg_finite(v.t, 3) || !std::isfinite(v.s) || !(v.s > 0)) return ORBG_BAD_ARG;
    F += v.fixed ? 0 : 1;
  }
  for (int k = 0; k < p->n_edges; k++) {
    const eg_edge& e = p->edges[k];
    if (e.vi < 0 || e.vi >= p->n_vertices || e.vj < 0 || e.vj >= p->n_vertices || e.vi == e.vj) return ORBG_BAD_ARG;
    if (!eg_finite(e.q, 4) || !eg_finite(e.t, 3) || !std::isfinite(e.s) || !(e.s > 0)) return ORBG_BAD_ARG;
  }
  for (int i = 0; i < p->n_points; i++) {
    const eg_point& x = p->points[i];
    if (x.ref >= p->n_vertices) return ORBG_BAD_ARG;
    if (!std::isfinite(x.pos[0]) || !std::isfinite(x.pos[1]) || !std::isfinite(x.pos[2])) return ORBG_BAD_ARG;
  }
  if (F > EG_MAX_FREE_KEYFRAMES) return ORBG_CAP_EXCEEDED;
  *n_free = F;
  return ORBG_OK;
}

inline S3 eg_s3(const double* q, const double* t, double s) { return S3{{q[0], q[1], q[2], q[3]}, {t[0], t[1], t[2]}, s}; }

struct EgRun {
  EgArea* const h;
  const hipStream_t st;
  const eg_problem* const p;
  eg_result* const r;
  LmScalars lm;
  const int NV, NE, NP, F, n;
  int n_pairs = 0, n_tasks = 0, n_blocks_lin = 0, n_blocks_e = 0;
  int cur = 0;
  const bool prof;
  std::vector<S3> s_est;
  std::vector<EgEdge> s_edges;
  std::vector<int> s_col, s_fixs, s_task_start, s_items, s_pair_i, s_pair_j;

  EgRun(EgArea* h_, const eg_problem* p_, eg_result* r_, int F_)
      : h(h_), st(h_ ? h_->stream : nullptr), p(p_), r(r_), NV(p_->n_vertices), NE(p_->n_edges), NP(p_->n_points), F(F_), n(7 * F_),
        prof(g_eg_profiling.load() != 0) {
    n_blocks_lin = (NE + kLinEdges - 1) / kLinEdges;
    n_blocks_e = (NE + 255) / 256;
  }

  void host_state() {
    s_est.resize((size_t)std::max(NV, 1));
    s_col.resize((size_t)std::max(NV, 1));
    s_fixs.resize((size_t)std::max(NV, 1));
    int c = 0;
    for (int i = 0; i < NV; i++) {
      const eg_vertex& v = p->vertices[i];
      s_est[i] = eg_s3(v.q, v.t, v.s);
      s_col[i] = v.fixed ? -1 : c++;
      s_fixs[i] = v.fix_scale ? 1 : 0;
    }
    s_edges.resize((size_t)std::max(NE, 1));
    for (int k = 0; k < NE; k++) {
      const eg_edge& e = p->edges[k];
      s_edges[k] = EgEdge{e.vi, e.vj, eg_s3(e.q, e.t, e.s)};
    }
  }

  // no free vertex, no edge or no iteration: nothing is launched; the estimates go back as they came, chi2 is evaluated here
  int finish_on_host() {
    double chi = 0;
    for (int k = 0; k < NE; k++) {
      double e[7];
      eg_error(s_edges[k].C, s_est[s_edges[k].vi], s_est[s_edges[k].vj], e);
      double c = 0;
      for (int a = 0; a < 7; a++) { c += e[a] * e[a]; if (r->edge_error0) r->edge_error0[7 * (size_t)k + a] = e[a]; }
      chi += c;
    }
    r->err0 = r->errEnd = chi;
    for (int i = 0; i < NV; i++) {
      double* o = r->estimates + 8 * (size_t)i;
      for (int a = 0; a < 4; a++) o[a] = s_est[i].q[a];
      for (int a = 0; a < 3; a++) o[4 + a] = s_est[i].t[a];
      o[7] = s_est[i].s;
    }
    for (int i = 0; i < NP; i++) {
      const eg_point& x = p->points[i];
      float* o = r->points + 3 * (size_t)i;
      if (x.ref < 0) { o[0] = x.pos[0]; o[1] = x.pos[1]; o[2] = x.pos[2]; continue; }
      S3 inv;
      s3_inverse(s_est[x.ref], &inv);
      const double P[3] = {(double)x.pos[0], (double)x.pos[1], (double)x.pos[2]};
      double a[3], b[3];
      s3_map(s_est[x.ref], P, a);
      s3_map(inv, a, b);
      o[0] = (float)b[0]; o[1] = (float)b[1]; o[2] = (float)b[2];
    }
    return ORBG_OK;
  }

  // per free vertex its items, then the distinct free-free pairs (row = the lower column) with theirs, all in edge order
  void structure() {
    std::vector<std::vector<int>> vitems((size_t)std::max(F, 1));
    std::map<std::pair<int, int>, int> pair_of;
    std::vector<std::vector<int>> pitems;
    for (int k = 0; k < NE; k++) {
      const int ci = s_col[s_edges[k].vi], cj = s_col[s_edges[k].vj];
      if (ci >= 0) vitems[ci].push_back(2 * k);
      if (cj >= 0) vitems[cj].push_back(2 * k + 1);
      if (ci < 0 || cj < 0) continue;
      const std::pair<int, int> key(std::min(ci, cj), std::max(ci, cj));
      auto it = pair_of.find(key);
      if (it == pair_of.end()) {
        it = pair_of.emplace(key, (int)pitems.size()).first;
        pitems.emplace_back();
        s_pair_i.push_back(key.first); s_pair_j.push_back(key.second);
      }
      pitems[it->second].push_back(2 * k + (ci < cj ? 0 : 1));
    }
    n_pairs = (int)pitems.size();
    n_tasks = F + n_pairs;
    s_task_start.assign((size_t)n_tasks + 1, 0);
    for (int t = 0; t < n_tasks; t++) {
      const std::vector<int>& v = t < F ? vitems[t] : pitems[t - F];
      s_items.insert(s_items.end(), v.begin(), v.end());
      s_task_start[t + 1] = (int)s_items.size();
    }
    if (s_items.empty()) s_items.push_back(0);
    if (s_pair_i.empty()) { s_pair_i.push_back(0); s_pair_j.push_back(0); }
  }

  int buffers() {
    int rc;
    h->ldlt.read_env();
    const size_t sNV = (size_t)std::max(NV, 1), sNE = (size_t)std::max(NE, 1), sF = (size_t)std::max(F, 1), sP = (size_t)std::max(n_pairs, 1);
    for (DevBuf<S3>& b : h->d_est) if ((rc = b.reserve(sNV))) return rc;
    if ((rc = h->d_edges.reserve(sNE)) || (rc = h->d_col.reserve(sNV)) || (rc = h->d_fixs.reserve(sNV)) ||
        (rc = h->d_task_start.reserve((size_t)n_tasks + 1)) || (rc = h->d_items.reserve(s_items.size())) || (rc = h->d_pair_i.reserve(sP)) ||
        (rc = h->d_pair_j.reserve(sP)) || (rc = h->d_ok.reserve(4)) || (rc = h->d_EJ.reserve(sNE * kEJ)) ||
        (rc = h->d_partial.reserve((size_t)std::max(n_blocks_lin, 1))) || (rc = h->d_Hd.reserve(49 * sF)) || (rc = h->d_bv.reserve(7 * sF)) ||
        (rc = h->d_Hp.reserve(49 * sP)) || (rc = h->d_x.reserve(7 * sF)) || (rc = h->d_scale_v.reserve(sNV)) || (rc = h->d_err0.reserve(7 * sNE)) ||
        (rc = h->d_pts.reserve((size_t)std::max(NP, 1))) || (rc = h->d_pts_out.reserve(3 * (size_t)std::max(NP, 1))) || (rc = h->d_rec.reserve(1)) ||
        (rc = h->rec.reserve(1)))
      return rc;
    if ((rc = h->ldlt.plan(n, st))) return rc;
    h->timer.on = prof;
    return h->timer.reset();
  }

  int upload() {
    // (pageable sources: hipMemcpyAsync returns once the bytes are staged)
    ORBG_HIP(hipMemcpyAsync(h->d_est[0].p, s_est.data(), sizeof(S3) * (size_t)NV, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_est[2].p, s_est.data(), sizeof(S3) * (size_t)NV, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_col.p, s_col.data(), sizeof(int) * (size_t)NV, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_fixs.p, s_fixs.data(), sizeof(int) * (size_t)NV, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_edges.p, s_edges.data(), sizeof(EgEdge) * (size_t)NE, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_task_start.p, s_task_start.data(), sizeof(int) * ((size_t)n_tasks + 1), hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_items.p, s_items.data(), sizeof(int) * s_items.size(), hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_pair_i.p, s_pair_i.data(), sizeof(int) * s_pair_i.size(), hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(h->d_pair_j.p, s_pair_j.data(), sizeof(int) * s_pair_j.size(), hipMemcpyHostToDevice, st));
    if (NP > 0) ORBG_HIP(hipMemcpyAsync(h->d_pts.p, p->points, sizeof(eg_point) * (size_t)NP, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipStreamSynchronize(st));
    return ORBG_OK;
  }

  int fetch_record() { return lm_fetch_record(h->rec.h, h->d_rec.p, st, h->timer); }

  // computeActiveErrors + buildSystem of state `buf`; the record brings chi2 and the largest diagonal entry
  int linearise(int buf) {
    h->timer.begin(kPhLin, st);
    hipLaunchKernelGGL(k_eg_lin, dim3(n_blocks_lin), dim3(256), 0, st, NE, h->d_edges.p, h->d_est[buf].p, h->d_col.p, h->d_fixs.p, h->d_EJ.p,
                       h->d_partial.p);
    h->timer.end(st);
    h->timer.begin(kPhAssemble, st);
    hipLaunchKernelGGL(k_eg_blocks, dim3(n_tasks), dim3(64), 0, st, F, h->d_task_start.p, h->d_items.p, h->d_EJ.p, h->d_Hd.p, h->d_bv.p, h->d_Hp.p);
    hipLaunchKernelGGL(k_eg_finish, dim3(1), dim3(256), 0, st, n_blocks_lin, h->d_partial.p, 0, h->d_scale_v.p, F, h->d_Hd.p, (const int*)nullptr,
                       h->d_rec.p);
    h->timer.end(st);
    return fetch_record();
  }

  // one trial: solve with lambda, trial state into buffer cur ^ 1, its chi2
  int trial(double lambda) {
    const int from = cur, to = cur ^ 1;
    int rc;
    h->timer.begin(kPhAssemble, st);
    if ((rc = h->ldlt.clear(h->d_x.p, st))) return rc;
    hipLaunchKernelGGL(k_eg_scatter, dim3(n_tasks), dim3(64), 0, st, F, h->d_pair_i.p, h->d_pair_j.p, h->d_Hd.p, h->d_bv.p, h->d_Hp.p, lambda,
                       h->ldlt.S(), h->ldlt.St());
    h->timer.end(st);
    h->timer.begin(kPhLdlt, st);
    if ((rc = h->ldlt.launch(h->d_bv.p, h->d_x.p, h->d_ok.p, st))) return rc;
    h->timer.end(st);
    h->timer.begin(kPhUpdate, st);
    hipLaunchKernelGGL(k_eg_update, dim3((NV + 255) / 256), dim3(256), 0, st, NV, h->d_col.p, h->d_fixs.p, h->d_est[from].p, h->d_x.p, h->d_bv.p, lambda,
                       h->d_ok.p, h->d_est[to].p, h->d_scale_v.p);
    hipLaunchKernelGGL(k_eg_errors, dim3(n_blocks_e), dim3(256), 0, st, NE, h->d_edges.p, h->d_est[to].p, h->d_partial.p, (double*)nullptr);
    hipLaunchKernelGGL(k_eg_finish, dim3(1), dim3(256), 0, st, n_blocks_e, h->d_partial.p, NV, h->d_scale_v.p, 0, (const double*)nullptr, h->d_ok.p,
                       h->d_rec.p);
    h->timer.end(st);
    return fetch_record();
  }

  // ---- what lm_optimize (lm_driver.hpp) asks of a solve; no stop flag here
  int linearise() { return linearise(cur); }
  const LmRec& record() const { return *h->rec.h; }
  int timed_out() const { return ldlt_timed_out_rc(h->rec.h->ok); }
  void accept() { cur ^= 1; }
  int first_linearisation(double* user_lambda) {
    *user_lambda = p->lambda_init;
    r->err0 = lm.currentChi;
    if (r->edge_error0) {                        // the error vectors of the initial estimate, as the linearisation stored them
      ORBG_HIP(hipMemcpy2DAsync(r->edge_error0, 7 * sizeof(double), h->d_EJ.p + 98, kEJ * sizeof(double), 7 * sizeof(double), (size_t)NE,
                                hipMemcpyDeviceToHost, st));
      ORBG_HIP(hipStreamSynchronize(st));
    }
    return ORBG_OK;
  }
  void iteration_done(int qmax, bool accepted) {
    r->errEnd = lm.currentChi;
    if (r->trace && r->trace_len < r->trace_cap) {
      double* t = r->trace + 4 * (size_t)r->trace_len;
      t[0] = qmax; t[1] = accepted ? 1 : 0; t[2] = lm.currentChi; t[3] = lm.lambda;
      r->trace_len++;
    }
  }

  int download() {
    if (NP > 0) {
      hipLaunchKernelGGL(k_eg_points, dim3((NP + 255) / 256), dim3(256), 0, st, NP, h->d_pts.p, h->d_est[2].p, h->d_est[cur].p, h->d_pts_out.p);
      ORBG_HIP(hipGetLastError());
      ORBG_HIP(hipMemcpyAsync(r->points, h->d_pts_out.p, sizeof(float) * 3 * (size_t)NP, hipMemcpyDeviceToHost, st));
    }
    static_assert(sizeof(S3) == 8 * sizeof(double), "an estimate goes back as eight doubles");
    ORBG_HIP(hipMemcpyAsync(r->estimates, h->d_est[cur].p, sizeof(S3) * (size_t)NV, hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipStreamSynchronize(st));
    return ORBG_OK;
  }
};

int eg_attempt(EgArea* h, EgRun& run) {
  int rc;
  StreamDrain drain{h->stream};
  run.cur = 0;
  run.lm = LmScalars();
  run.r->trace_len = 0;
  if ((rc = run.buffers()) || (rc = run.upload())) return rc;
  int done = 0;
  StopCheck no_flag;
  if ((rc = lm_optimize(run, run.p->iterations, no_flag, &done))) return rc;
  run.r->iters = done;
  rc = run.download();
  h->timer.flush(h->stream);
  if (run.prof) for (int i = 0; i < 4; i++) t_eg_phase_ms[i] = h->timer.ms[i];
  return rc;
}

}  // namespace

extern "C" int eg_solve(const eg_problem* p, eg_result* r) {
  int F = 0;
  int rc = eg_validate(p, r, &F);
  if (rc) return rc;
  r->iters = 0; r->trace_len = 0; r->err0 = r->errEnd = 0;
  if (F == 0 || p->n_edges == 0 || p->iterations <= 0) {
    EgRun run(nullptr, p, r, F);                 // host arrays only: no device is selected, no stream created
    run.host_state();
    return run.finish_on_host();
  }
  static thread_local EgArea area;
  if ((rc = area.open(p->device, "misc"))) return rc;
  EgRun run(&area, p, r, F);
  run.host_state();
  run.structure();
  // (a timed-out launch: solved again on the one-workgroup kernels, which this thread then keeps using)
  return ldlt_retry(area.ldlt, area.stream, [&] { return eg_attempt(&area, run); });
}

extern "C" int eg_set_profiling(int on) {
  g_eg_profiling.store(on ? 1 : 0);
  return ORBG_OK;
}
extern "C" int eg_get_phase_ms(double* ms) {
  if (!ms) return ORBG_BAD_ARG;
  for (int i = 0; i < 4; i++) ms[i] = t_eg_phase_ms[i];
  return ORBG_OK;
}
