// Reference-signature glue of the server's loop closing above the C ABI (include/orbgpu.h): header-only templates over the reference's
// own types, as include/orbgpu_dropin.hpp and include/orbgpu_localmapping.hpp are for theirs.
//
//   void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
//                                          const KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections,
//                                          const bool& bFixScale)                            I/Optimizer.h, S/Optimizer.cc:2413-2747
//     -> orbgpu::loopclosing::OptimizeEssentialGraph(...), same arguments in the same order (call site: S/LoopClosing.cc:1272)
//
// The forms at S/Optimizer.cc:3196 (MergeLocal) and :3596 build the same eg_problem from other keyframe sets; their
// glue is not provided.
//
// Matrices: the including translation unit declares, BEFORE this header, in namespace orbgpu::loopclosing
//   const float* mat_f32(const MatT&);                                  the float32 elements of a continuous matrix
//   void make_mat(MatT& out, int rows, int cols, const float* data);    a new rows x cols CV_32F matrix
// (for cv::Mat: `return m.ptr<float>(0);` and `out = cv::Mat(rows, cols, CV_32F); memcpy(out.data, data, 4 * rows * cols);`).
//
// Pinned deviations from the reference, each marked at its line below:
//   D-1  A bad keyframe has no vertex (:2449).  The reference then hands a null vertex to an edge (:2513, :2566 and the other setVertex
//        calls) or dereferences one in the write-back (:2694).  Here such an edge is dropped, such a write-back skipped, both counted.
//   D-2  pKF->bImu && pKF->mPrevKF (:2646): std::logic_error.  The inertial edge is not part of this entry point.
#pragma once

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#include "orbgpu.h"

namespace orbgpu {
namespace loopclosing {

// ---- g2o::Sim3 on the host, as far as the collection needs it (G/types/sim3.h): the same statements, in the same order, as the
// library's own (multi_orbslam3_amd/csrc/sim3_math.hpp) and the checker's (tests/sim3_opt_model.py, choices E-1, E-2, E-3, E-6, E-7)
struct S3 { double q[4], t[3], s; };

inline void quat_rotate(const double* q, const double* v, double* out) {
  const double uv0 = 2 * (q[1] * v[2] - q[2] * v[1]), uv1 = 2 * (q[2] * v[0] - q[0] * v[2]), uv2 = 2 * (q[0] * v[1] - q[1] * v[0]);
  out[0] = v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1);
  out[1] = v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2);
  out[2] = v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0);
}
inline S3 s3_mul(const S3& a, const S3& b) {                       // sim3.h:266-272
  S3 o;
  const double* x = a.q; const double* y = b.q;
  o.q[0] = x[3] * y[0] + x[0] * y[3] + x[1] * y[2] - x[2] * y[1];
  o.q[1] = x[3] * y[1] + x[1] * y[3] + x[2] * y[0] - x[0] * y[2];
  o.q[2] = x[3] * y[2] + x[2] * y[3] + x[0] * y[1] - x[1] * y[0];
  o.q[3] = x[3] * y[3] - x[0] * y[0] - x[1] * y[1] - x[2] * y[2];
  double rt[3];
  quat_rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) o.t[i] = a.s * rt[i] + a.t[i];
  o.s = a.s * b.s;
  return o;
}
inline S3 s3_inverse(const S3& a) {                                // sim3.h:233-236
  S3 o;
  o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
  const double k = -1. / a.s;
  const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
  quat_rotate(o.q, v, o.t);
  o.s = 1. / a.s;
  return o;
}
inline S3 s3_identity() { return S3{{0, 0, 0, 1}, {0, 0, 0}, 1}; }  // Sim3(): sim3.h:49-54
// g2o::Sim3(Rcw, tcw, 1.0) (sim3.h:64-67): Eigen::Quaterniond(Matrix3d), not renormalised
inline S3 s3_from_pose(const float* R /* 3 x 3 */, const float* t) {
  const double m[9] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]};
  S3 o;
  double* q = o.q;
  double tr = m[0] + m[4] + m[8];
  if (tr > 0) {
    tr = std::sqrt(tr + 1.0);
    q[3] = 0.5 * tr;
    tr = 0.5 / tr;
    q[0] = (m[7] - m[5]) * tr; q[1] = (m[2] - m[6]) * tr; q[2] = (m[3] - m[1]) * tr;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    tr = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
    q[i] = 0.5 * tr;
    tr = 0.5 / tr;
    q[3] = (m[3 * k + j] - m[3 * j + k]) * tr;
    q[j] = (m[3 * j + i] + m[3 * i + j]) * tr;
    q[k] = (m[3 * k + i] + m[3 * i + k]) * tr;
  }
  o.t[0] = t[0]; o.t[1] = t[1]; o.t[2] = t[2];
  o.s = 1.0;
  return o;
}
template <class Sim3T> inline S3 s3_of(const Sim3T& S) {
  S3 o;
  for (int i = 0; i < 4; i++) o.q[i] = S.rotation().coeffs()[i];
  for (int i = 0; i < 3; i++) o.t[i] = S.translation()[i];
  o.s = S.scale();
  return o;
}

struct GpuOps {
  static int eg(const eg_problem& p, eg_result& r) { return eg_solve(&p, &r); }
};

struct EssentialGraphReport {
  int n_vertices = 0, n_edges = 0, n_points = 0;
  int dropped_edges = 0;          // D-1: an end without a vertex
  int skipped_write_backs = 0;    // D-1: keyframes without a vertex at :2694
  int iters = 0;
  double err0 = 0, errEnd = 0;
};

template <class Ops = GpuOps, class MapT, class KeyFrameT, class KeyFrameAndPoseT, class LoopConnectionsT>
EssentialGraphReport OptimizeEssentialGraph(MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const KeyFrameAndPoseT& NonCorrectedSim3,
                                            const KeyFrameAndPoseT& CorrectedSim3, const LoopConnectionsT& LoopConnections, const bool& bFixScale,
                                            int device = 0) {
  EssentialGraphReport rep;
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMPs = pMap->GetAllMapPoints();
  const int minFeat = 100;                                                       // :2443

  // ---- vertices (:2446-2483): ascending mnUniqueId, g2o's order of the free vertices' columns
  std::vector<std::pair<long unsigned, KeyFrameT*>> order;
  for (KeyFrameT* pKF : vpKFs)
    if (!pKF->isBad()) order.emplace_back(pKF->mnUniqueId, pKF);                 // D-1 (:2449)
  std::sort(order.begin(), order.end());
  std::map<long unsigned, int> vertex_of;                                        // mnUniqueId -> vertex (optimizer.vertex(nIDi))
  std::vector<eg_vertex> vertices(order.size());
  std::vector<S3> vScw(order.size());
  for (size_t n = 0; n < order.size(); n++) {
    KeyFrameT* pKF = order[n].second;
    const auto it = CorrectedSim3.find(pKF);
    S3 S;
    if (it != CorrectedSim3.end()) S = s3_of(it->second);                        // :2458-2462
    else {
      const auto R = pKF->GetRotation();
      const auto t = pKF->GetTranslation();
      S = s3_from_pose(mat_f32(R), mat_f32(t));                                  // :2465-2469
    }
    vScw[n] = S;
    eg_vertex& v = vertices[n];
    for (int i = 0; i < 4; i++) v.q[i] = S.q[i];
    for (int i = 0; i < 3; i++) v.t[i] = S.t[i];
    v.s = S.s;
    v.fixed = pKF->mnId == pMap->GetInitKFid() ? 1 : 0;                          // :2472
    v.fix_scale = bFixScale ? 1 : 0;                                             // :2477
    vertex_of[pKF->mnUniqueId] = (int)n;
  }
  auto vertex = [&](KeyFrameT* pKF) { const auto it = vertex_of.find(pKF->mnUniqueId); return it == vertex_of.end() ? -1 : it->second; };
  // vScw[nID] of the reference: the vertex's estimate, or the default-constructed identity of a keyframe without one (:2435)
  auto Scw = [&](KeyFrameT* pKF) { const int v = vertex(pKF); return v < 0 ? s3_identity() : vScw[v]; };
  auto non_corrected = [&](KeyFrameT* pKF) {
    const auto it = NonCorrectedSim3.find(pKF);
    return it != NonCorrectedSim3.end() ? s3_of(it->second) : Scw(pKF);
  };

  std::vector<eg_edge> edges;
  auto add_edge = [&](KeyFrameT* pKFi, KeyFrameT* pKFj, const S3& Sji) {
    const int vi = vertex(pKFi), vj = vertex(pKFj);
    if (vi < 0 || vj < 0) { rep.dropped_edges++; return; }                       // D-1 (:2513-2514, :2566-2567, :2596-2597, :2634-2635)
    eg_edge e;
    e.vi = vi; e.vj = vj;
    for (int i = 0; i < 4; i++) e.q[i] = Sji.q[i];
    for (int i = 0; i < 3; i++) e.t[i] = Sji.t[i];
    e.s = Sji.s;
    edges.push_back(e);
  };

  // ---- loop edges (:2492-2523)
  std::set<std::pair<long unsigned, long unsigned>> sInsertedEdges;
  for (auto mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {
    KeyFrameT* pKF = mit->first;
    const long unsigned nIDi = pKF->mnUniqueId;
    const S3 Swi = s3_inverse(Scw(pKF));
    for (auto sit = mit->second.begin(); sit != mit->second.end(); ++sit) {
      const long unsigned nIDj = (*sit)->mnUniqueId;
      if ((nIDi != pCurKF->mnUniqueId || nIDj != pLoopKF->mnUniqueId) && pKF->GetWeight(*sit) < minFeat) continue;      // :2506
      add_edge(pKF, *sit, s3_mul(Scw(*sit), Swi));
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }

  // ---- normal edges (:2530-2666); like the reference, the loop does not skip bad keyframes: their edges are dropped by D-1
  for (KeyFrameT* pKF : vpKFs) {
    const S3 Swi = s3_inverse(non_corrected(pKF));                               // :2539-2544
    KeyFrameT* pParentKF = pKF->GetParent();
    if (pParentKF) add_edge(pKF, pParentKF, s3_mul(non_corrected(pParentKF), Swi));          // :2549-2573
    const auto sLoopEdges = pKF->GetLoopEdges();
    for (auto sit = sLoopEdges.begin(); sit != sLoopEdges.end(); ++sit) {        // :2576-2604
      KeyFrameT* pLKF = *sit;
      if (pLKF->mnUniqueId < pKF->mnUniqueId) add_edge(pKF, pLKF, s3_mul(non_corrected(pLKF), Swi));
    }
    const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);             // :2607-2643
    for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); ++vit) {
      KeyFrameT* pKFn = *vit;
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnUniqueId < pKF->mnUniqueId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnUniqueId, pKFn->mnUniqueId), std::max(pKF->mnUniqueId, pKFn->mnUniqueId))))
            continue;
          add_edge(pKF, pKFn, s3_mul(non_corrected(pKFn), Swi));
        }
      }
    }
    if (pKF->bImu && pKF->mPrevKF)                                               // D-2 (:2646)
      throw std::logic_error("orbgpu::loopclosing::OptimizeEssentialGraph: the inertial edge of S/Optimizer.cc:2646 is not provided");
  }

  // ---- map points (:2711-2733): the vertex whose estimates they go through
  std::vector<eg_point> points;
  std::vector<size_t> point_index;
  for (size_t i = 0; i < vpMPs.size(); i++) {
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    long unsigned nIDr;
    if (pMP->mnCorrectedByKF == pCurKF->mnUniqueId) nIDr = pMP->mnCorrectedReference;       // :2720-2723
    else nIDr = pMP->GetReferenceKeyFrame()->mnUniqueId;
    const auto it = vertex_of.find(nIDr);
    eg_point x;
    const auto P3Dw = pMP->GetWorldPos();
    const float* X = mat_f32(P3Dw);
    x.pos[0] = X[0]; x.pos[1] = X[1]; x.pos[2] = X[2];
    x.ref = it == vertex_of.end() ? -1 : it->second;                             // two identities in the reference: the point keeps its bits
    points.push_back(x);
    point_index.push_back(i);
  }

  // ---- optimize (:2677-2682)
  std::vector<double> estimates(8 * std::max<size_t>(vertices.size(), 1));
  std::vector<float> corrected(3 * std::max<size_t>(points.size(), 1));
  eg_problem p{};
  p.struct_size = sizeof(eg_problem);
  p.n_vertices = (int32_t)vertices.size(); p.vertices = vertices.data();
  p.n_edges = (int32_t)edges.size(); p.edges = edges.data();
  p.iterations = 20;                                                             // :2680
  p.lambda_init = 1e-16;                                                         // :2426
  p.n_points = (int32_t)points.size(); p.points = points.data();
  p.device = device;
  eg_result r{};
  r.struct_size = sizeof(eg_result);
  r.estimates = estimates.data(); r.points = corrected.data();
  const int rc = Ops::eg(p, r);
  if (rc != ORBG_OK) throw std::runtime_error("orbgpu::loopclosing::OptimizeEssentialGraph: eg_solve failed (there is no CPU path)");
  rep.n_vertices = p.n_vertices; rep.n_edges = p.n_edges; rep.n_points = p.n_points;
  rep.iters = r.iters; rep.err0 = r.err0; rep.errEnd = r.errEnd;

  // ---- write-back (:2684-2746)
  std::unique_lock<typename std::remove_reference<decltype(pMap->mMutexMapUpdate)>::type> lock(pMap->mMutexMapUpdate);      // :2684 (std::mutex)
  for (KeyFrameT* pKFi : vpKFs) {
    const int v = vertex(pKFi);
    if (v < 0) { rep.skipped_write_backs++; continue; }                          // D-1 (:2694)
    const double* e = &estimates[8 * (size_t)v];
    // eigR = CorrectedSiw.rotation().toRotationMatrix(); eigt *= (1. / s); Converter::toCvSE3 (:2697-2703)
    const double tx = 2 * e[0], ty = 2 * e[1], tz = 2 * e[2];
    const double twx = tx * e[3], twy = ty * e[3], twz = tz * e[3];
    const double txx = tx * e[0], txy = ty * e[0], txz = tz * e[0];
    const double tyy = ty * e[1], tyz = tz * e[1], tzz = tz * e[2];
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    const double inv_s = 1. / e[7];
    float T[16];
    for (int a = 0; a < 3; a++) {
      for (int c = 0; c < 3; c++) T[4 * a + c] = (float)R[3 * a + c];
      T[4 * a + 3] = (float)(e[4 + a] * inv_s);
    }
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
    auto Tiw = pKFi->GetRotation();                                              // (a matrix of the reference's type to assign to)
    make_mat(Tiw, 4, 4, T);
    pKFi->SetPose(Tiw, true);                                                    // :2705
  }
  for (size_t n = 0; n < points.size(); n++) {
    auto* pMP = vpMPs[point_index[n]];
    auto cvCorrectedP3Dw = pMP->GetWorldPos();
    make_mat(cvCorrectedP3Dw, 3, 1, &corrected[3 * n]);
    pMP->SetWorldPos(cvCorrectedP3Dw, true);                                     // :2740
    pMP->UpdateNormalAndDepth();                                                 // :2742, on the host
  }
  pMap->IncreaseChangeIndex();                                                   // :2746
  return rep;
}

}  // namespace loopclosing
}  // namespace orbgpu
