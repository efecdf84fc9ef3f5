// Drop-in glue for the optimisers of an inertial agent (INTEGRATION.md sections 3n, 3o): templates over the reference's own types.
//
//   int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame *pFrame, bool bRecInit = false)   I/Optimizer.h, S/Optimizer.cc:7603-7996
//   int Optimizer::PoseInertialOptimizationLastFrame(Frame *pFrame, bool bRecInit = false)      I/Optimizer.h, S/Optimizer.cc:7998-8424
//   void Optimizer::LocalInertialBA(KeyFrame *pKF, bool *pbStopFlag, Map *pMap, bool bLarge, bool bRecInit)   S/Optimizer.cc:4556-5226
//   void Optimizer::InertialOptimization(...), four overloads                                               S/Optimizer.cc:5344-5958
//
// Collect what :7659-7815 / :8040-8226 read, call pose_inertial_optimize (include/orbgpu.h), write back what :7949-7993 / :8361-8421
// write.  Matrices are read through mat_f32(m) (a const float* to row-major data, found by argument-dependent lookup or the cv::Mat
// overload below) and written through make_mat(m, rows, cols, data).  A ConstraintPoseImu is read through operator() of its members
// (Eigen) and built by a factory: EigenConstraintFactory calls the reference's constructor, which conditions H itself.
#ifndef ORBGPU_INERTIAL_HPP_
#define ORBGPU_INERTIAL_HPP_

#include <cstdint>
#include <cstring>
#include <algorithm>
#include <cmath>
#include <list>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "orbgpu.h"

namespace orbgpu {
namespace inertial {

#ifdef HAVE_OPENCV
inline const float* mat_f32(const cv::Mat& m) { return m.ptr<float>(0); }
inline void make_mat(cv::Mat& out, int rows, int cols, const float* data) { out = cv::Mat(rows, cols, CV_32F, const_cast<float*>(data)).clone(); }
#endif

// the library calls; a test replaces them to look at what the glue hands over
struct GpuOps {
  static int optimize(const pose_inertial_problem& p, pose_inertial_result& r) { return pose_inertial_optimize(&p, &r); }
  static int information(const float* C, double* i9, double* ig, double* ia) { return orbg_imu_information(C, i9, ig, ia); }
};

#ifdef EIGEN_WORLD_VERSION
// new ConstraintPoseImu(Rwb, twb, vwb, bg, ba, H) as S/Optimizer.cc:7993, 8419 call it
struct EigenConstraintFactory {
  template <class CpiT>
  static CpiT* make(const pose_inertial_result& r) {
    Eigen::Matrix3d R; Eigen::Vector3d t, v, bg, ba; Eigen::Matrix<double, 15, 15> H;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R(i, j) = r.Rwb[3 * i + j]; t(i) = r.twb[i]; v(i) = r.vwb[i]; bg(i) = r.bg[i]; ba(i) = r.ba[i]; }
    for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) H(i, j) = r.H[15 * i + j];
    return new CpiT(R, t, v, bg, ba, H);
  }
};
typedef EigenConstraintFactory DefaultConstraintFactory;
#else
struct NoConstraintFactory {};
typedef NoConstraintFactory DefaultConstraintFactory;
#endif

inline void check(int rc, const char* where) {
  if (rc != ORBG_OK) throw std::runtime_error(std::string("orbgpu inertial: ") + where + " failed: " + orbg_strerror(rc));
}

template <class M> inline void read_state_mats(const M& R, const M& t, const M& v, pose_inertial_state* s) {
  std::memcpy(s->Rwb, mat_f32(R), sizeof(s->Rwb)); std::memcpy(s->twb, mat_f32(t), sizeof(s->twb)); std::memcpy(s->vwb, mat_f32(v), sizeof(s->vwb));
}
// VertexPose / Velocity / GyroBias / AccBias of a Frame (S/G2oTypes.cc:73-119, 664-691)
template <class FrameT> inline void read_frame_state(FrameT* F, pose_inertial_state* s) {
  read_state_mats(F->GetImuRotation(), F->GetImuPosition(), F->mVw, s);
  s->bg[0] = F->mImuBias.bwx; s->bg[1] = F->mImuBias.bwy; s->bg[2] = F->mImuBias.bwz;
  s->ba[0] = F->mImuBias.bax; s->ba[1] = F->mImuBias.bay; s->ba[2] = F->mImuBias.baz;
}
// ... of a KeyFrame (S/G2oTypes.cc:27-71, 659-683)
template <class KeyFrameT> inline void read_keyframe_state(KeyFrameT* K, pose_inertial_state* s) {
  read_state_mats(K->GetImuRotation(), K->GetImuPosition(), K->GetVelocity(), s);
  const auto g = K->GetGyroBias(); const auto a = K->GetAccBias();
  std::memcpy(s->bg, mat_f32(g), sizeof(s->bg)); std::memcpy(s->ba, mat_f32(a), sizeof(s->ba));
}
template <class PreT> inline void read_preintegration(const PreT* I, pose_inertial_preint* o) {
  o->dT = I->dT;
  std::memcpy(o->dR, mat_f32(I->dR), 36); std::memcpy(o->dV, mat_f32(I->dV), 12); std::memcpy(o->dP, mat_f32(I->dP), 12);
  std::memcpy(o->JRg, mat_f32(I->JRg), 36); std::memcpy(o->JVg, mat_f32(I->JVg), 36); std::memcpy(o->JVa, mat_f32(I->JVa), 36);
  std::memcpy(o->JPg, mat_f32(I->JPg), 36); std::memcpy(o->JPa, mat_f32(I->JPa), 36);
  o->bg[0] = I->b.bwx; o->bg[1] = I->b.bwy; o->bg[2] = I->b.bwz; o->ba[0] = I->b.bax; o->ba[1] = I->b.bay; o->ba[2] = I->b.baz;
}
template <class CpiT> inline void read_constraint(const CpiT& c, pose_inertial_prior* o) {
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) o->Rwb[3 * i + j] = c.Rwb(i, j); o->twb[i] = c.twb(i); o->vwb[i] = c.vwb(i); o->bg[i] = c.bg(i); o->ba[i] = c.ba(i); }
  for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) o->H[15 * i + j] = c.H(i, j);
}

template <class Ops, class Factory, class FrameT>
int optimize(FrameT* pFrame, bool bRecInit, int form) {
  if (pFrame->Nleft != -1 || pFrame->mpCamera2) throw std::runtime_error("orbgpu inertial: a two-camera Frame is not supported");
  const bool last_frame = form == POSE_INERTIAL_LAST_FRAME;
  typedef typename std::remove_pointer<decltype(pFrame->mpcpi)>::type CpiT;
  pose_inertial_problem P;
  std::memset(&P, 0, sizeof(P));
  P.struct_size = sizeof(P); P.form = form; P.rec_init = bRecInit ? 1 : 0; P.device = 0; P.n_left = -1;
  // the visual edges (:7659-7764, :8040-8158): one per feature with a map point, mvKeysUn, mvuRight < 0 => monocular
  const int N = pFrame->N;
  std::vector<float> Xw, u, v, ur, w; std::vector<uint8_t> close; std::vector<int> featIdx;
  for (int i = 0; i < N; i++) {
    auto* pMP = pFrame->mvpMapPoints[i];
    if (!pMP) continue;
    pFrame->mvbOutlier[i] = false;
    const auto& kp = pFrame->mvKeysUn[i];
    const auto Xm = pMP->GetWorldPos();
    const float* X = mat_f32(Xm);
    Xw.insert(Xw.end(), X, X + 3); u.push_back(kp.pt.x); v.push_back(kp.pt.y); ur.push_back(pFrame->mvuRight[i]);
    w.push_back(pFrame->mvInvLevelSigma2[kp.octave]); close.push_back(pMP->mTrackDepth < 10.f ? 1 : 0); featIdx.push_back(i);
  }
  P.n = (int32_t)featIdx.size();
  P.Xw = Xw.data(); P.u = u.data(); P.v = v.data(); P.ur = ur.data(); P.inv_sigma2 = w.data(); P.close = close.data();
  P.fx = pFrame->fx; P.fy = pFrame->fy; P.cx = pFrame->cx; P.cy = pFrame->cy; P.bf = pFrame->mbf;
  std::memcpy(P.Tcb, mat_f32(pFrame->mImuCalib.Tcb), sizeof(P.Tcb));
  read_frame_state(pFrame, &P.frame);
  // the other end and its preintegration (:7767-7815, :8163-8212)
  const auto* pInt = last_frame ? pFrame->mpImuPreintegratedFrame : pFrame->mpImuPreintegrated;
  if (!pInt) throw std::runtime_error("orbgpu inertial: the Frame has no preintegration");
  pose_inertial_prior prior;
  if (last_frame) {
    auto* pFp = pFrame->mpPrevFrame;
    if (!pFp) throw std::runtime_error("orbgpu inertial: the Frame has no previous frame");
    if (!pFp->mpcpi) throw std::runtime_error("orbgpu inertial: pFp->mpcpi does not exist");     // (the reference dereferences NULL at :8217)
    read_frame_state(pFp, &P.other);
    read_constraint(*pFp->mpcpi, &prior);
    P.prior = &prior;
  } else {
    if (!pFrame->mpLastKeyFrame) throw std::runtime_error("orbgpu inertial: the Frame has no last keyframe");
    read_keyframe_state(pFrame->mpLastKeyFrame, &P.other);
  }
  read_preintegration(pInt, &P.preint);
  check(Ops::information(mat_f32(pInt->C), P.info9, P.infoG, P.infoA), "orbg_imu_information");
  std::vector<uint8_t> outlier(featIdx.size() + 1);
  pose_inertial_result R;
  std::memset(&R, 0, sizeof(R));
  R.struct_size = sizeof(R); R.outlier = outlier.data();
  check(Ops::optimize(P, R), last_frame ? "PoseInertialOptimizationLastFrame" : "PoseInertialOptimizationLastKeyFrame");
  // write back (:7949-7993, :8361-8421)
  for (size_t k = 0; k < featIdx.size(); k++) pFrame->mvbOutlier[featIdx[k]] = outlier[k] != 0;
  float Rf[9], tf[3], vf[3];
  for (int i = 0; i < 9; i++) Rf[i] = (float)R.Rwb[i];
  for (int i = 0; i < 3; i++) { tf[i] = (float)R.twb[i]; vf[i] = (float)R.vwb[i]; }
  typename std::decay<decltype(pFrame->mVw)>::type mR, mt, mv;
  make_mat(mR, 3, 3, Rf); make_mat(mt, 3, 1, tf); make_mat(mv, 3, 1, vf);
  pFrame->SetImuPoseVelocity(mR, mt, mv);
  typedef typename std::decay<decltype(pFrame->mImuBias)>::type BiasT;
  pFrame->mImuBias = BiasT((float)R.ba[0], (float)R.ba[1], (float)R.ba[2], (float)R.bg[0], (float)R.bg[1], (float)R.bg[2]);   // IMU::Bias takes (ba, bg)
  pFrame->mpcpi = Factory::template make<CpiT>(R);
  if (last_frame) {
    auto* pFp = pFrame->mpPrevFrame;
    delete pFp->mpcpi;
    pFp->mpcpi = nullptr;
  }
  return R.n_inliers;
}

}  // namespace inertial

template <class Ops = inertial::GpuOps, class Factory = inertial::DefaultConstraintFactory, class FrameT>
int PoseInertialOptimizationLastKeyFrame(FrameT* pFrame, bool bRecInit = false) {
  return inertial::optimize<Ops, Factory>(pFrame, bRecInit, POSE_INERTIAL_LAST_KEYFRAME);
}
template <class Ops = inertial::GpuOps, class Factory = inertial::DefaultConstraintFactory, class FrameT>
int PoseInertialOptimizationLastFrame(FrameT* pFrame, bool bRecInit = false) {
  return inertial::optimize<Ops, Factory>(pFrame, bRecInit, POSE_INERTIAL_LAST_FRAME);
}

// ---------------------------------------------------------------------------------------------- LocalInertialBA
namespace inertial {

// the library calls of the local inertial BA; a test replaces them to look at what the glue hands over and to force the fail return
struct LibaGpuOps {
  static int solve(const inertial_ba_problem& p, inertial_ba_result& r) { return inertial_ba_solve(&p, &r); }
  static int information(const float* C, double* i9, double* ig, double* ia) { return orbg_imu_information(C, i9, ig, ia); }
};

// VertexPose of a KeyFrame (S/G2oTypes.cc:27-71), and with bImu its velocity and biases (:659-683)
template <class KeyFrameT> inline void read_liba_state(KeyFrameT* K, pose_inertial_state* s) {
  std::memset(s, 0, sizeof(*s));
  const auto R = K->GetImuRotation(); const auto t = K->GetImuPosition();
  std::memcpy(s->Rwb, mat_f32(R), sizeof(s->Rwb)); std::memcpy(s->twb, mat_f32(t), sizeof(s->twb));
  if (!K->bImu) return;
  const auto v = K->GetVelocity(); const auto g = K->GetGyroBias(); const auto a = K->GetAccBias();
  std::memcpy(s->vwb, mat_f32(v), sizeof(s->vwb)); std::memcpy(s->bg, mat_f32(g), sizeof(s->bg)); std::memcpy(s->ba, mat_f32(a), sizeof(s->ba));
}

}  // namespace inertial

// The window, the stamps, the point list and the fixed list in the reference's order, the SetNewBias side effect, inertial_ba_solve,
// the erase list (mono edges first, then stereo), the lock, the fail return with its un-reset stamps, the write-back in the
// reference's order.  pbStopFlag is accepted and not read: the reference hands it to the optimizer after optimize() has returned
// (:5077).  A keyframe with mpCamera2 throws (EdgeMono(1) is not part of inertial_ba_solve).
template <class Ops = inertial::LibaGpuOps, class KeyFrameT, class MapT>
void LocalInertialBA(KeyFrameT* pKF, bool* pbStopFlag, MapT* pMap, bool bLarge = false, bool bRecInit = false) {
  using namespace inertial;
  (void)pbStopFlag;
  auto* pCurrentMap = pKF->GetMap();
  const int maxOpt = bLarge ? 25 : 10;
  const int Nd = std::min((int)pCurrentMap->KeyFramesInMap() - 2, maxOpt);
  typedef typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches())>::type::value_type>::type MapPointT;
  // the window (:4571-4587)
  std::vector<KeyFrameT*> vpOptimizableKFs;
  vpOptimizableKFs.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  for (int i = 1; i < Nd; i++) {
    if (!vpOptimizableKFs.back()->mPrevKF) break;
    vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
    vpOptimizableKFs.back()->mnBALocalForKF = pKF->mnId;
  }
  int N = (int)vpOptimizableKFs.size();
  // the points its keyframes see (:4592-4607)
  std::vector<MapPointT*> lLocalMapPoints;
  for (int i = 0; i < N; i++) {
    const auto vpMPs = vpOptimizableKFs[i]->GetMapPointMatches();
    for (MapPointT* pMP : vpMPs)
      if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) { lLocalMapPoints.push_back(pMP); pMP->mnBALocalForKF = pKF->mnId; }
  }
  // the fixed keyframe in front of the window -- or the oldest one itself, popped (:4610-4622)
  std::list<KeyFrameT*> lFixedKeyFrames;
  if (vpOptimizableKFs.back()->mPrevKF) {
    lFixedKeyFrames.push_back(vpOptimizableKFs.back()->mPrevKF);
    vpOptimizableKFs.back()->mPrevKF->mnBAFixedForKF = pKF->mnId;
  } else {
    vpOptimizableKFs.back()->mnBALocalForKF = 0;
    vpOptimizableKFs.back()->mnBAFixedForKF = pKF->mnId;
    lFixedKeyFrames.push_back(vpOptimizableKFs.back());
    vpOptimizableKFs.pop_back();
  }
  // (maxCovKF = 0: the loop of :4626-4654 leaves at its first test)
  // the other observers of the local points, one per point at most, up to 200 keyframes in all (:4657-4678)
  const size_t maxFixKF = 200;
  for (MapPointT* pMP : lLocalMapPoints) {
    const auto observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrameT* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad()) { lFixedKeyFrames.push_back(pKFi); break; }
      }
    }
    if (lFixedKeyFrames.size() >= maxFixKF) break;
  }
  // the vertices (:4704-4775): the window first, then the fixed list
  N = (int)vpOptimizableKFs.size();
  std::vector<KeyFrameT*> all(vpOptimizableKFs.begin(), vpOptimizableKFs.end());
  all.insert(all.end(), lFixedKeyFrames.begin(), lFixedKeyFrames.end());
  std::map<KeyFrameT*, int> index;
  std::vector<inertial_ba_keyframe> kfs(all.size());
  for (size_t i = 0; i < all.size(); i++) {
    std::memset(&kfs[i], 0, sizeof(kfs[i]));
    read_liba_state(all[i], &kfs[i].state);
    kfs[i].fixed = (int)i >= N ? 1 : 0; kfs[i].imu = all[i]->bImu ? 1 : 0; kfs[i].prev = -1;
    index[all[i]] = (int)i;
  }
  // the inertial edges (:4782-4867)
  for (int i = 0; i < N; i++) {
    KeyFrameT* pKFi = vpOptimizableKFs[i];
    if (!pKFi->mPrevKF) continue;
    if (!(pKFi->bImu && pKFi->mPrevKF->bImu && pKFi->mpImuPreintegrated)) continue;
    pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());
    const auto it = index.find(pKFi->mPrevKF);
    if (it == index.end()) continue;                              // (:4811: a vertex is missing)
    inertial_ba_keyframe& k = kfs[i];
    k.link = 1; k.prev = it->second; k.last_in_window = i == N - 1 ? 1 : 0;
    read_preintegration(pKFi->mpImuPreintegrated, &k.preint);
    check(Ops::information(mat_f32(pKFi->mpImuPreintegrated->C), k.info9, k.infoG, k.infoA), "orbg_imu_information");
  }
  // the points and their edges (:4914-5059)
  std::vector<float> points; std::vector<uint8_t> close; std::vector<lba_edge> edges;
  std::vector<KeyFrameT*> vpEdgeKF; std::vector<MapPointT*> vpMapPointEdge;
  for (MapPointT* pMP : lLocalMapPoints) {
    const auto Xm = pMP->GetWorldPos();
    const float* X = mat_f32(Xm);
    const int l = (int)close.size();
    points.insert(points.end(), X, X + 3);
    close.push_back(pMP->mTrackDepth < 10.f ? 1 : 0);
    const auto observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrameT* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) continue;
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      if (pKFi->mpCamera2) throw std::runtime_error("orbgpu inertial: a two-camera KeyFrame is not supported");
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex == -1) continue;
      const auto& kpUn = pKFi->mvKeysUn[leftIndex];
      lba_edge e;
      e.pose = index.at(pKFi); e.point = l; e.u = kpUn.pt.x; e.v = kpUn.pt.y;
      e.ur = pKFi->mvuRight[leftIndex] < 0 ? -1.f : pKFi->mvuRight[leftIndex];
      e.inv_sigma2 = pKFi->mvInvLevelSigma2[kpUn.octave];          // (Pinhole::uncertainty2 is 1)
      edges.push_back(e); vpEdgeKF.push_back(pKFi); vpMapPointEdge.push_back(pMP);
    }
  }
  inertial_ba_problem P;
  std::memset(&P, 0, sizeof(P));
  P.struct_size = sizeof(P); P.n_keyframes = (int32_t)kfs.size(); P.n_points = (int32_t)close.size(); P.n_edges = (int32_t)edges.size();
  P.keyframes = kfs.data(); P.points = points.data(); P.edges = edges.data(); P.close = close.data();
  P.rec_init = bRecInit ? 1 : 0; P.large = bLarge ? 1 : 0; P.device = 0;
  P.fx = pKF->fx; P.fy = pKF->fy; P.cx = pKF->cx; P.cy = pKF->cy; P.bf = pKF->mbf;
  std::memcpy(P.Tcb, mat_f32(pKF->mImuCalib.Tcb), sizeof(P.Tcb));
  std::vector<inertial_ba_state> states(kfs.size());
  std::vector<float> new_points(points.size() + 1);
  std::vector<uint8_t> outlier(edges.size() + 1);
  inertial_ba_result R;
  std::memset(&R, 0, sizeof(R));
  R.struct_size = sizeof(R); R.states = states.data(); R.points = new_points.data(); R.edge_outlier = outlier.data();
  check(Ops::solve(P, R), "LocalInertialBA");
  // the erase list (:5083-5119): the mono edges in their order, then the stereo edges
  std::vector<std::pair<KeyFrameT*, MapPointT*> > vToErase;
  for (int stereo = 0; stereo < 2; stereo++)
    for (size_t k = 0; k < edges.size(); k++) {
      if ((edges[k].ur < 0) == (stereo == 1) || vpMapPointEdge[k]->isBad()) continue;
      if (outlier[k]) vToErase.push_back(std::make_pair(vpEdgeKF[k], vpMapPointEdge[k]));
    }
  std::unique_lock<typename std::decay<decltype(pMap->mMutexMapUpdate)>::type> lock(pMap->mMutexMapUpdate);
  if (R.failed) return;                                           // (:5128-5132: the stamps stay as they are, nothing is written)
  for (auto& er : vToErase) { er.first->EraseMapPointMatch(er.second); er.second->EraseObservation(er.first); }
  for (KeyFrameT* pKFi : lFixedKeyFrames) pKFi->mnBAFixedForKF = 0;
  // write-back (:5157-5213)
  typedef typename std::decay<decltype(pKF->GetImuBias())>::type BiasT;
  typedef typename std::decay<decltype(pKF->GetVelocity())>::type MatT;
  const float* Tcb = P.Tcb;
  for (int i = 0; i < N; i++) {
    KeyFrameT* pKFi = vpOptimizableKFs[i];
    const inertial_ba_state& s = states[i];
    if (pKFi->bImu) {
      const float vf[3] = {(float)s.vwb[0], (float)s.vwb[1], (float)s.vwb[2]};
      MatT mv;
      make_mat(mv, 3, 1, vf);
      pKFi->SetVelocity(mv);
      pKFi->SetNewBias(BiasT((float)s.ba[0], (float)s.ba[1], (float)s.ba[2], (float)s.bg[0], (float)s.bg[1], (float)s.bg[2]));   // IMU::Bias takes (ba, bg)
    }
    // Rcw = Rcb Rwb^T, tcw = Rcb (-Rwb^T twb) + tcb in double (ImuCamPose), then Converter::toCvSE3: floats
    double Rcb[9], tcb[3], tbw[3];
    for (int a = 0; a < 3; a++) { for (int c = 0; c < 3; c++) Rcb[3 * a + c] = Tcb[4 * a + c]; tcb[a] = Tcb[4 * a + 3]; }
    for (int a = 0; a < 3; a++) tbw[a] = -(s.Rwb[a] * s.twb[0] + s.Rwb[3 + a] * s.twb[1] + s.Rwb[6 + a] * s.twb[2]);
    float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    for (int a = 0; a < 3; a++) {
      for (int c = 0; c < 3; c++) T[4 * a + c] = (float)(Rcb[3 * a] * s.Rwb[3 * c] + Rcb[3 * a + 1] * s.Rwb[3 * c + 1] + Rcb[3 * a + 2] * s.Rwb[3 * c + 2]);
      T[4 * a + 3] = (float)(Rcb[3 * a] * tbw[0] + Rcb[3 * a + 1] * tbw[1] + Rcb[3 * a + 2] * tbw[2] + tcb[a]);
    }
    MatT mT;
    make_mat(mT, 4, 4, T);
    pKFi->SetPose(mT, false);
    pKFi->mnBALocalForKF = 0;
  }
  for (size_t l = 0; l < lLocalMapPoints.size(); l++) {
    MatT mX;
    make_mat(mX, 3, 1, &new_points[3 * l]);
    lLocalMapPoints[l]->SetWorldPos(mX, false, false);
    lLocalMapPoints[l]->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}

// ---------------------------------------------------------------------------------------------- InertialOptimization
//   void Optimizer::InertialOptimization(Map*, Eigen::Matrix3d &Rwg, double &scale, Eigen::Vector3d &bg, Eigen::Vector3d &ba, bool bMono,
//                                        Eigen::MatrixXd &covInertial, bool bFixedVel, bool bGauss, float priorG, float priorA)   S/Optimizer.cc:5344
//   void Optimizer::InertialOptimization(Map*, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA)              :5534
//   void Optimizer::InertialOptimization(vector<KeyFrame*>, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA) :5696
//   void Optimizer::InertialOptimization(Map*, Eigen::Matrix3d &Rwg, double &scale)                                               :5858
namespace inertial {

// the library calls of the inertial initialisation; a test replaces them to look at what the glue hands over
struct InitGpuOps {
  static int solve(const inertial_init_problem& p, inertial_init_result& r) { return inertial_init_solve(&p, &r); }
  static int information(const float* C, double* i9, double* ig, double* ia) { return orbg_imu_information(C, i9, ig, ia); }
};

// What the four overloads share.  P comes in with its switches set.  Vertices: every keyframe of the list (map_filter: those with mnId <=
// maxKFid), found again by mnId as g2o finds them.  Edges: a keyframe with an mPrevKF and mnId <= maxKFid, neither bad nor behind a
// predecessor beyond maxKFid; set_bias: the SetNewBias(mPrevKF->GetImuBias()) side effect of the first three overloads, applied BEFORE
// the vertices are looked up, so also to an edge that is then skipped because its predecessor is not in the list (:5782-5796).  Every
// bias vertex is constructed from vpKFs.front().  Returns the velocities per listed keyframe (index as in `listed`).
template <class Ops, class KeyFrameT>
struct InitSolve {
  std::vector<KeyFrameT*> listed;
  std::vector<double> vwb;
  inertial_init_result R;
  void run(const std::vector<KeyFrameT*>& vpKFs, unsigned long maxKFid, bool map_filter, bool set_bias, inertial_init_problem& P) {
    if (vpKFs.empty()) throw std::runtime_error("orbgpu inertial: InertialOptimization without keyframes");
    std::map<unsigned long, int> index;
    std::vector<pose_inertial_state> kfs;
    for (KeyFrameT* pKFi : vpKFs) {
      if (map_filter && pKFi->mnId > maxKFid) continue;
      pose_inertial_state s;
      read_keyframe_state(pKFi, &s);
      index[pKFi->mnId] = (int)kfs.size();
      kfs.push_back(s); listed.push_back(pKFi);
    }
    std::vector<inertial_init_edge> edges;
    for (KeyFrameT* pKFi : vpKFs) {
      if (!(pKFi->mPrevKF && pKFi->mnId <= maxKFid)) continue;
      if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
      if (!pKFi->mpImuPreintegrated) throw std::runtime_error("orbgpu inertial: a keyframe has no preintegration");   // (the reference dereferences NULL)
      if (set_bias) pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());
      const auto i1 = index.find(pKFi->mPrevKF->mnId), i2 = index.find(pKFi->mnId);
      if (i1 == index.end() || i2 == index.end()) continue;                        // a vertex is missing
      inertial_init_edge e;
      std::memset(&e, 0, sizeof(e));
      e.k1 = i1->second; e.k2 = i2->second;
      read_preintegration(pKFi->mpImuPreintegrated, &e.preint);
      double ig[9], ia[9];
      check(Ops::information(mat_f32(pKFi->mpImuPreintegrated->C), e.info9, ig, ia), "orbg_imu_information");
      edges.push_back(e);
    }
    const auto g = vpKFs.front()->GetGyroBias(); const auto a = vpKFs.front()->GetAccBias();
    std::memcpy(P.bg, mat_f32(g), sizeof(P.bg)); std::memcpy(P.ba, mat_f32(a), sizeof(P.ba));
    P.struct_size = sizeof(P); P.device = 0;
    P.n_keyframes = (int32_t)kfs.size(); P.keyframes = kfs.data(); P.n_edges = (int32_t)edges.size(); P.edges = edges.data();
    vwb.assign(3 * kfs.size() + 3, 0.0);
    std::memset(&R, 0, sizeof(R));
    R.struct_size = sizeof(R); R.vwb = vwb.data();
    check(Ops::solve(P, R), "InertialOptimization");
    R.vwb = nullptr;
  }
  // :5506-5530: SetVelocity, then SetNewBias -- behind a Reintegrate() when the gyro bias moved by more than 0.01 (cv::norm of a float
  // difference, summed in double)
  void write_back(unsigned long maxKFid) {
    typedef typename std::decay<decltype(listed[0]->GetImuBias())>::type BiasT;
    typedef typename std::decay<decltype(listed[0]->GetVelocity())>::type MatT;
    const BiasT b((float)R.ba[0], (float)R.ba[1], (float)R.ba[2], (float)R.bg[0], (float)R.bg[1], (float)R.bg[2]);   // IMU::Bias takes (ba, bg)
    for (size_t i = 0; i < listed.size(); i++) {
      KeyFrameT* pKFi = listed[i];
      if (pKFi->mnId > maxKFid) continue;
      const float vf[3] = {(float)vwb[3 * i], (float)vwb[3 * i + 1], (float)vwb[3 * i + 2]};
      MatT mv;
      make_mat(mv, 3, 1, vf);
      pKFi->SetVelocity(mv);
      const auto og = pKFi->GetGyroBias();
      const float* o = mat_f32(og);
      double n2 = 0;
      for (int k = 0; k < 3; k++) { const float d = o[k] - (float)R.bg[k]; n2 += (double)d * (double)d; }
      pKFi->SetNewBias(b);
      if (std::sqrt(n2) > 0.01 && pKFi->mpImuPreintegrated) pKFi->mpImuPreintegrated->Reintegrate();
    }
  }
};

inline void init_switches(inertial_init_problem* P, int algorithm, int its, double lambda, bool v, bool b, bool g, bool s, bool priors, float priorG, float priorA) {
  std::memset(P, 0, sizeof(*P));
  P->algorithm = algorithm; P->iterations = its; P->lambda_init = lambda;
  P->free_velocity = v; P->free_bias = b; P->free_gdir = g; P->free_scale = s;
  P->with_priors = priors; P->prior_g = (double)priorG; P->prior_a = (double)priorA;
  P->Rwg[0] = P->Rwg[4] = P->Rwg[8] = 1.0; P->scale = 1.0;
}

}  // namespace inertial

// covInertial is accepted and not touched, bGauss is not read: the reference reads neither.
template <class Ops = inertial::InitGpuOps, class MapT, class Mat3T, class Vec3T, class CovT>
void InertialOptimization(MapT* pMap, Mat3T& Rwg, double& scale, Vec3T& bg, Vec3T& ba, bool bMono, CovT& covInertial, bool bFixedVel = false,
                          bool bGauss = false, float priorG = 1e2, float priorA = 1e6) {
  using namespace inertial;
  (void)covInertial; (void)bGauss;
  const unsigned long maxKFid = pMap->GetMaxKFid();
  const auto vpKFs = pMap->GetAllKeyFrames();
  typedef typename std::remove_pointer<typename std::decay<decltype(vpKFs)>::type::value_type>::type KeyFrameT;
  inertial_init_problem P;
  init_switches(&P, INERTIAL_INIT_LM, 200, priorG != 0.f ? 1e3 : 0.0, !bFixedVel, !bFixedVel, true, bMono, true, priorG, priorA);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) P.Rwg[3 * i + j] = Rwg(i, j);
  P.scale = scale;
  InitSolve<Ops, KeyFrameT> S;
  S.run(vpKFs, maxKFid, true, true, P);
  scale = S.R.scale;
  for (int i = 0; i < 3; i++) { bg(i) = S.R.bg[i]; ba(i) = S.R.ba[i]; for (int j = 0; j < 3; j++) Rwg(i, j) = S.R.Rwg[3 * i + j]; }
  S.write_back(maxKFid);
}

namespace inertial {
template <class Ops, class KeyFrameT, class Vec3T>
void init_bias_only(const std::vector<KeyFrameT*>& vpKFs, unsigned long maxKFid, bool map_filter, Vec3T& bg, Vec3T& ba, float priorG, float priorA) {
  inertial_init_problem P;
  init_switches(&P, INERTIAL_INIT_LM, 200, 1e3, true, true, false, false, true, priorG, priorA);
  InitSolve<Ops, KeyFrameT> S;
  S.run(vpKFs, maxKFid, map_filter, true, P);
  for (int i = 0; i < 3; i++) { bg(i) = S.R.bg[i]; ba(i) = S.R.ba[i]; }
  S.write_back(maxKFid);
}
}  // namespace inertial

template <class Ops = inertial::InitGpuOps, class MapT, class Vec3T>
void InertialOptimization(MapT* pMap, Vec3T& bg, Vec3T& ba, float priorG = 1e2, float priorA = 1e6) {
  const unsigned long maxKFid = pMap->GetMaxKFid();
  const auto vpKFs = pMap->GetAllKeyFrames();
  typedef typename std::remove_pointer<typename std::decay<decltype(vpKFs)>::type::value_type>::type KeyFrameT;
  inertial::init_bias_only<Ops, KeyFrameT>(vpKFs, maxKFid, true, bg, ba, priorG, priorA);
}

// the list's keyframes all get vertices, beyond maxKFid too (:5716-5731: the filter is commented out); an edge whose predecessor is not
// in the list is skipped (:5791)
template <class Ops = inertial::InitGpuOps, class KeyFrameT, class Vec3T>
void InertialOptimization(std::vector<KeyFrameT*> vpKFs, Vec3T& bg, Vec3T& ba, float priorG = 1e2, float priorA = 1e6) {
  if (vpKFs.empty()) throw std::runtime_error("orbgpu inertial: InertialOptimization without keyframes");
  const unsigned long maxKFid = vpKFs[0]->GetMap()->GetMaxKFid();
  inertial::init_bias_only<Ops, KeyFrameT>(vpKFs, maxKFid, false, bg, ba, priorG, priorA);
}

// Gauss-Newton on the gravity direction and the scale alone; no keyframe is written
template <class Ops = inertial::InitGpuOps, class MapT, class Mat3T>
void InertialOptimization(MapT* pMap, Mat3T& Rwg, double& scale) {
  using namespace inertial;
  const unsigned long maxKFid = pMap->GetMaxKFid();
  const auto vpKFs = pMap->GetAllKeyFrames();
  typedef typename std::remove_pointer<typename std::decay<decltype(vpKFs)>::type::value_type>::type KeyFrameT;
  inertial_init_problem P;
  init_switches(&P, INERTIAL_INIT_GN, 10, 0.0, false, false, true, true, false, 0.f, 0.f);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) P.Rwg[3 * i + j] = Rwg(i, j);
  P.scale = scale;
  InitSolve<Ops, KeyFrameT> S;
  S.run(vpKFs, maxKFid, true, false, P);
  scale = S.R.scale;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rwg(i, j) = S.R.Rwg[3 * i + j];
}

}  // namespace orbgpu

#endif  // ORBGPU_INERTIAL_HPP_
