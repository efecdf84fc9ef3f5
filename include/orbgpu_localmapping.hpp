// LocalMapping::CreateNewMapPoints (S/LocalMapping.cc:520-865) over liborbgpu: a function template with the body of the reference's
// member function, duck-typed on the reference's member names, to be called from LocalMapping::CreateNewMapPoints in place of its
// body ("CreateNewMapPoints").  Everything that is private to LocalMapping (CheckNewKeyFrames, the MapPoint
// constructor's arguments, mpAtlas, mlpRecentAddedMapPoints) comes in through three callables.
//
// What runs where:
//   host    the neighbour list with the inertial mPrevKF extension (:527-540), the baseline / ComputeSceneMedianDepth gates (:573-590),
//           the upload (or reuse) of the device keyframes, and per created point the reference's :847-862.
//   device  SearchForTriangulation + triangulation of ALL neighbours that passed the gates: ONE orbm_create_new_points call.
// The loop's early exit (`i > 0 && CheckNewKeyFrames()`, :566) is honoured at neighbour boundaries: the list comes back in the
// reference's creation order, points are applied neighbour by neighbour, and CheckNewKeyFrames() is asked before each neighbour
// i > 0 exactly as the reference asks it; when it says so the rest of the list is discarded.  The reference would not have computed
// that rest; nothing of it has been applied.
//
// Scope: keyframes of a rig (mpCamera2 != NULL, NLeft != -1) or with a camera that is not a Pinhole cannot be passed to the library:
// the function returns -1 before it has changed anything and the caller runs the reference's body.
// bCoarse (:597-599) is evaluated by the caller once per call (the reference re-evaluates the same expression per neighbour).
// Every member read here is public in I/KeyFrame.h (N, mvKeys, mvKeysUn, mvuRight, mvDepth, mDescriptors, mFeatVec, fx .. invfy, mb,
// mbf, mvScaleFactors, mvLevelSigma2, mfScaleFactor, mnScaleLevels, mnMinX .. mnMaxY, mpCamera, mpCamera2, NLeft, mPrevKF, and the
// getters GetPose / GetPoseInverse / GetCameraCenter / GetMapPointMatches / GetBestCovisibilityKeyFrames / ComputeSceneMedianDepth /
// AddMapPoint): no reference-side edit is needed.
#ifndef ORBGPU_LOCALMAPPING_HPP_
#define ORBGPU_LOCALMAPPING_HPP_

#include <algorithm>
#include <cmath>
#include <memory>
#include <unordered_map>
#include <vector>

#include "orbgpu_dropin.hpp"

namespace orbgpu {

// The device-resident copies of keyframes (a KeyFrame's features never change after its construction): uploaded on first use, reused
// by later calls (the current keyframe of one call is a neighbour of the next ones).  One per LocalMapping thread; Erase() when a
// keyframe is deleted.
template <class KeyFrameT>
class KeyFramesOnDevice {
 public:
  explicit KeyFramesOnDevice(int device = 0) : device_(device) {}
  FrameOnDevice& Get(KeyFrameT* pKF) {
    auto it = frames_.find(pKF);
    if (it != frames_.end()) return *it->second;
    const int N = pKF->N;
    std::vector<orbx_keypoint> kps(N);
    std::vector<uint8_t> desc((size_t)N * 32);
    for (int i = 0; i < N; i++) {
      const auto& kp = pKF->mvKeysUn[i];
      kps[i] = orbx_keypoint{kp.pt.x, kp.pt.y, kp.size, kp.angle, kp.response, (int32_t)kp.octave};
      std::memcpy(&desc[(size_t)32 * i], dropin::mat_u8(pKF->mDescriptors, i), 32);
    }
    std::unique_ptr<FrameOnDevice> f(new FrameOnDevice(std::max(N, 1), device_));
    f->Upload(orbm_frame_view{N, kps.data(), desc.data(), pKF->mvuRight.data(), pKF->mvDepth.data(), (float)pKF->mnMinX, (float)pKF->mnMaxX,
                              (float)pKF->mnMinY, (float)pKF->mnMaxY, pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf, pKF->mb,
                              pKF->mnScaleLevels, pKF->mfScaleFactor});
    return *(frames_[pKF] = std::move(f));
  }
  void Erase(KeyFrameT* pKF) { frames_.erase(pKF); }
  size_t size() const { return frames_.size(); }
 private:
  int device_;
  std::unordered_map<KeyFrameT*, std::unique_ptr<FrameOnDevice>> frames_;
};

namespace localmapping {

template <class KeyFrameT>
struct KfSide {                 // what one orbm_newpoints_kf points at
  std::vector<uint8_t> has_mp;
  std::vector<float> keys_xy;
  std::unique_ptr<dropin::FeatVecFlat<decltype(KeyFrameT::mFeatVec)>> fv;
};

template <class KeyFrameT>
inline bool in_scope(KeyFrameT* pKF) {
  return !pKF->mpCamera2 && pKF->NLeft == -1 && pKF->mpCamera && pKF->mpCamera->GetType() == ORBG_CAM_PINHOLE;
}

template <class KeyFrameT>
inline void fill_side(KeyFrameT* pKF, FrameOnDevice& dev, KfSide<KeyFrameT>& s, orbm_newpoints_kf& k) {
  const int N = pKF->N;
  const auto vpMP = pKF->GetMapPointMatches();
  s.has_mp.resize(N);
  for (int i = 0; i < N; i++) s.has_mp[i] = vpMP[i] != nullptr;                   // GetMapPoint(idx) != NULL, bad points included
  bool distorted = false;                                                          // UnprojectStereo reads mvKeys (S/KeyFrame.cc:952-953)
  for (int i = 0; i < N && !distorted; i++) distorted = pKF->mvKeys[i].pt.x != pKF->mvKeysUn[i].pt.x || pKF->mvKeys[i].pt.y != pKF->mvKeysUn[i].pt.y;
  if (distorted) {
    s.keys_xy.resize((size_t)2 * N);
    for (int i = 0; i < N; i++) { s.keys_xy[2 * i] = pKF->mvKeys[i].pt.x; s.keys_xy[2 * i + 1] = pKF->mvKeys[i].pt.y; }
  }
  s.fv.reset(new dropin::FeatVecFlat<decltype(KeyFrameT::mFeatVec)>(pKF->mFeatVec));
  k.struct_size = sizeof(orbm_newpoints_kf);
  k.frame = dev.handle();
  k.featvec = s.fv->v;
  k.has_mp = s.has_mp.data();
  k.keys_xy = distorted ? s.keys_xy.data() : nullptr;
  const auto Tcw = pKF->GetPose(), Twc = pKF->GetPoseInverse(), Ow = pKF->GetCameraCenter();
  std::memcpy(k.Tcw, dropin::mat_f32(Tcw), sizeof(k.Tcw));                         // rows 0-2 of the 4 x 4
  std::memcpy(k.Twc, dropin::mat_f32(Twc), sizeof(k.Twc));
  std::memcpy(k.Ow, dropin::mat_f32(Ow), sizeof(k.Ow));
  k.fx = pKF->fx; k.fy = pKF->fy; k.cx = pKF->cx; k.cy = pKF->cy; k.invfx = pKF->invfx; k.invfy = pKF->invfy; k.mb = pKF->mb; k.mbf = pKF->mbf;
  k.n_levels = (int32_t)pKF->mvScaleFactors.size();
  k.scale_factors = pKF->mvScaleFactors.data();
  k.level_sigma2 = pKF->mvLevelSigma2.data();
  k.scale_factor = pKF->mfScaleFactor;
}

}  // namespace localmapping

// The body of LocalMapping::CreateNewMapPoints.  mbMonocular / mbInertial / mbFarPoints / mThFarPoints: the LocalMapping members;
// bCoarse: :597-599.  CheckNewKeyFrames: bool().  NewMapPoint: MapPointT*(const MatT& x3D, KeyFrameT* pRefKF) -- `new MapPoint(x3D,
// mpCurrentKeyFrame, mpAtlas->GetCurrentMap(), ...)`, :847.  AddToMap: void(MapPointT*) -- mpAtlas->AddMapPoint(pMP) and
// mlpRecentAddedMapPoints.push_back(pMP), :861-862.  Returns the number of points created, or -1 when a keyframe is out of scope
// (nothing has been changed: run the reference's body).
template <class MatT, class KeyFrameT, class CheckFn, class NewFn, class AddFn>
int CreateNewMapPoints(KeyFrameT* mpCurrentKeyFrame, KeyFramesOnDevice<KeyFrameT>& onDevice, bool mbMonocular, bool mbInertial, bool bCoarse,
                       bool mbFarPoints, float mThFarPoints, CheckFn CheckNewKeyFrames, NewFn NewMapPoint, AddFn AddToMap) {
  // Retrieve neighbor keyframes in covisibility graph
  int nn = 10;
  if (mbMonocular) nn = 20;
  std::vector<KeyFrameT*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  if (mbInertial) {
    KeyFrameT* pKF = mpCurrentKeyFrame;
    int count = 0;
    while (((int)vpNeighKFs.size() <= nn) && (pKF->mPrevKF) && (count++ < nn)) {
      auto it = std::find(vpNeighKFs.begin(), vpNeighKFs.end(), pKF->mPrevKF);
      if (it == vpNeighKFs.end()) vpNeighKFs.push_back(pKF->mPrevKF);
      pKF = pKF->mPrevKF;
    }
  }
  if (!localmapping::in_scope(mpCurrentKeyFrame)) return -1;
  for (KeyFrameT* pKF2 : vpNeighKFs)
    if (!localmapping::in_scope(pKF2)) return -1;

  // Check first that baseline is not too short (:573-590); `kept` = the neighbours SearchForTriangulation is called for
  const auto Ow1m = mpCurrentKeyFrame->GetCameraCenter();
  const float* Ow1 = dropin::mat_f32(Ow1m);
  std::vector<int> kept;
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    KeyFrameT* pKF2 = vpNeighKFs[i];
    const auto Ow2m = pKF2->GetCameraCenter();
    const float* Ow2 = dropin::mat_f32(Ow2m);
    const float v[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
    const float baseline = (float)std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);   // cv::norm: double accumulation
    if (!mbMonocular) {
      if (baseline < pKF2->mb) continue;
    } else {
      const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
      const float ratioBaselineDepth = baseline / medianDepthKF2;
      if (ratioBaselineDepth < 0.01) continue;
    }
    kept.push_back((int)i);
  }

  const int B = (int)kept.size();
  std::vector<orbm_newpoint> created;
  int n_created = 0;
  if (B > 0 && mpCurrentKeyFrame->N > 0) {
    localmapping::KfSide<KeyFrameT> side1;
    std::vector<localmapping::KfSide<KeyFrameT>> sides(B);
    orbm_newpoints_kf k1{};
    std::vector<orbm_newpoints_kf> kn(B);
    localmapping::fill_side(mpCurrentKeyFrame, onDevice.Get(mpCurrentKeyFrame), side1, k1);
    for (int b = 0; b < B; b++) { kn[b] = orbm_newpoints_kf{}; localmapping::fill_side(vpNeighKFs[kept[b]], onDevice.Get(vpNeighKFs[kept[b]]), sides[b], kn[b]); }
    orbm_newpoints_params p{};
    p.struct_size = sizeof(p);
    p.only_stereo = 0; p.coarse = bCoarse; p.check_orientation = 0;              // ORBmatcher matcher(0.6f, false), :544; bOnlyStereo = false, :600
    p.far_points = mbFarPoints; p.th_far_points = mThFarPoints;
    created.resize((size_t)mpCurrentKeyFrame->N);                                // a feature of the current keyframe gets at most one point
    check(orbm_create_new_points(&k1, kn.data(), B, &p, created.data(), (int)created.size(), &n_created, nullptr, nullptr), "orbm_create_new_points");
  }

  // Apply the list neighbour by neighbour, asking CheckNewKeyFrames() where the reference's loop asks it (:566)
  int made = 0, at = 0, b = 0;
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    if (i > 0 && CheckNewKeyFrames()) return made;
    if (b >= B || kept[b] != (int)i) continue;                                   // a neighbour the baseline gate left out
    KeyFrameT* pKF2 = vpNeighKFs[i];
    for (; at < n_created && created[at].neighbour == b; at++) {
      const orbm_newpoint& c = created[at];
      MatT x3D;
      dropin::make_mat(x3D, 3, 1, c.x3D);
      auto* pMP = NewMapPoint(x3D, mpCurrentKeyFrame);                           // Triangulation is succesfull, :847
      pMP->AddObservation(mpCurrentKeyFrame, c.idx1);
      pMP->AddObservation(pKF2, c.idx2);
      mpCurrentKeyFrame->AddMapPoint(pMP, c.idx1);
      pKF2->AddMapPoint(pMP, c.idx2);
      pMP->ComputeDistinctiveDescriptors();
      pMP->UpdateNormalAndDepth();
      AddToMap(pMP);
      made++;
    }
    b++;
  }
  return made;
}

}  // namespace orbgpu

#endif  // ORBGPU_LOCALMAPPING_HPP_
