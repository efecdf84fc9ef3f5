// The per-keyframe steps of LocalMapping::RunClient over liborbgpu: CreateNewMapPoints (below) and SearchInNeighbors / Fuse (second
// half of this file).
//
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
#include <cstring>
#include <memory>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
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

// ------------------------------------------------------------------------------------------------ Fuse / SearchInNeighbors
// ORBmatcher::Fuse(pKF, vpMapPoints, th) (S/ORBmatcher.cc:1395-1605, bRight = false) and LocalMapping::SearchInNeighbors
// (S/LocalMapping.cc:868-976) over liborbgpu.
//
// What runs where:
//   device  everything of a (keyframe, point) pair up to bestIdx / bestDist, against the state at entry: orbm_fuse, ONE launch for all
//           the target keyframes of direction one, ONE for direction two (the current keyframe against the targets' points).
//   host    the target list (:871-917), the replay of :1431-1448 and :1569-1590 over the real objects in the reference's order, the
//           gathering of vpFuseCandidates (:937-953), the update loop (:959-972) and UpdateConnections().
// The only input of a pair that changes while the replay runs is the point's descriptor (MapPoint::Replace ends in
// ComputeDistinctiveDescriptors on the survivor).  The replay compares GetDescriptor() with the 32 bytes the launch saw; where they
// differ it rescores over the record's candidate list (first strict minimum from bestDist = 256), and where that list is longer than
// ORBG_FUSE_CAND_CAP it re-evaluates the single pair (orbm_fuse with K = 1, P = 1).  Positions, normals and distance ranges do not
// change before the update loop.
//
// Scope: as CreateNewMapPoints -- a rig keyframe (NLeft != -1, mpCamera2) or a camera that is not a Pinhole among the targets or the
// current keyframe makes SearchInNeighbors return -1 before it has written anything; the caller then runs the reference's body.
// Members read: KeyFrame mnId, mnFuseTargetForKF, isBad, GetBestCovisibilityKeyFrames, mPrevKF, GetMapPointMatches, GetMapPoint,
// AddMapPoint, GetPose, GetCameraCenter, UpdateConnections, fx .. mbf, N, mvKeysUn, mvuRight, mvDepth, mDescriptors, mnScaleLevels,
// mfScaleFactor, mfLogScaleFactor, mvScaleFactors, mvInvLevelSigma2, mnMinX .. mnMaxY, mpCamera, mpCamera2, NLeft; MapPoint isBad,
// IsInKeyFrame, GetWorldPos, GetNormal, GetDescriptor, Observations, Replace, AddObservation, ComputeDistinctiveDescriptors,
// UpdateNormalAndDepth, mnFuseCandidateForKF -- all public in the reference -- and the raw distance range through
// dropin::min_distance_raw / max_distance_raw (INTEGRATION.md edit E1, which the Tracking glue needs already; no further edit).

struct FuseStats { long pairs = 0, rescored = 0, relaunched = 0; };   // records replayed / rescored on the host / re-evaluated singly

namespace localmapping {

constexpr int TH_LOW = 50;        // S/ORBmatcher.cc:37

template <class KeyFrameT>
inline void fill_fuse_kf(KeyFrameT* pKF, FrameOnDevice& dev, orbm_fuse_kf& k) {
  k = orbm_fuse_kf{};
  k.struct_size = sizeof(orbm_fuse_kf);
  k.frame = dev.handle();
  const auto Tcw = pKF->GetPose(), Ow = pKF->GetCameraCenter();
  std::memcpy(k.Tcw, dropin::mat_f32(Tcw), sizeof(k.Tcw));                         // rows 0-2 of the 4 x 4: GetRotation() | GetTranslation()
  std::memcpy(k.Ow, dropin::mat_f32(Ow), sizeof(k.Ow));
  k.fx = pKF->fx; k.fy = pKF->fy; k.cx = pKF->cx; k.cy = pKF->cy; k.mbf = pKF->mbf;
  k.n_levels = (int32_t)pKF->mvScaleFactors.size();
  k.scale_factors = pKF->mvScaleFactors.data();
  k.inv_level_sigma2 = pKF->mvInvLevelSigma2.data();
  k.log_scale_factor = pKF->mfLogScaleFactor;
}

// the points of one launch, flat: entry i is vpMapPoints[i] (a NULL entry stays zero and is skipped)
template <class MapPointT>
struct FusePoints {
  std::vector<float> pos, normal, min_dist, max_dist;
  std::vector<uint8_t> desc;
  orbm_worldpoints_view view{};
  explicit FusePoints(const std::vector<MapPointT*>& v) : pos(3 * v.size()), normal(3 * v.size()), min_dist(v.size()), max_dist(v.size()), desc(32 * v.size()) {
    for (size_t i = 0; i < v.size(); i++) {
      MapPointT* p = v[i];
      if (!p) continue;
      const auto X = p->GetWorldPos(); const auto nv = p->GetNormal(); const auto D = p->GetDescriptor();
      std::memcpy(&pos[3 * i], dropin::mat_f32(X), 12); std::memcpy(&normal[3 * i], dropin::mat_f32(nv), 12);
      min_dist[i] = dropin::min_distance_raw(p, 0); max_dist[i] = dropin::max_distance_raw(p, 0);
      std::memcpy(&desc[32 * i], dropin::mat_u8(D, 0), 32);
    }
    view.m = (int32_t)v.size();
    view.pos = pos.data(); view.normal = normal.data(); view.min_dist = min_dist.data(); view.max_dist = max_dist.data(); view.desc = desc.data();
  }
};

inline int hamming256(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int w = 0; w < 4; w++) { uint64_t x, y; std::memcpy(&x, a + 8 * w, 8); std::memcpy(&y, b + 8 * w, 8); d += __builtin_popcountll(x ^ y); }
  return d;
}

// K keyframes x the points of vpMapPoints in one launch.  skip[k * P + i]: NULL, bad or already in keyframe k at entry.
template <class KeyFrameT, class MapPointT>
struct FuseLaunch {
  int K, P;
  FusePoints<MapPointT> pts;
  std::vector<orbm_fuse_kf> kfs;
  std::vector<orbm_fuse_record> rec;
  std::vector<uint16_t> cand;
  std::vector<uint8_t> skip;        // NULL, bad or already in keyframe k at entry: conditions that only ever become true
  float th;
  FuseLaunch(const std::vector<KeyFrameT*>& targets, const std::vector<MapPointT*>& vpMapPoints, float th_, KeyFramesOnDevice<KeyFrameT>& onDevice)
      : K((int)targets.size()), P((int)vpMapPoints.size()), pts(vpMapPoints), kfs(targets.size()), rec((size_t)K * P), cand((size_t)K * P * ORBG_FUSE_CAND_CAP), skip((size_t)K * P), th(th_) {
    if (K == 0 || P == 0) return;
    for (int k = 0; k < K; k++) {
      fill_fuse_kf(targets[k], onDevice.Get(targets[k]), kfs[k]);
      for (int i = 0; i < P; i++) {
        MapPointT* p = vpMapPoints[i];
        skip[(size_t)k * P + i] = !p || p->isBad() || p->IsInKeyFrame(targets[k]);
      }
    }
    orbm_fuse_params prm{};
    prm.struct_size = sizeof(prm); prm.th = th; prm.sim3_form = 0;
    check(orbm_fuse(kfs.data(), K, &pts.view, skip.data(), &prm, rec.data(), cand.data()), "orbm_fuse");
  }

  // the loop :1427-1592 for keyframe k over the records; returns nFused
  int Replay(int k, KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, FuseStats* stats) {
    int nFused = 0;
    for (int i = 0; i < P; i++) {
      if (skip[(size_t)k * P + i]) continue;                          // skipped at entry stays skipped: the reference's two locked
      MapPointT* pMP = vpMapPoints[i];                                // calls per pair are made once for such a pair, not twice
      if (pMP->isBad()) continue;
      else if (pMP->IsInKeyFrame(pKF)) continue;
      const orbm_fuse_record& r = rec[(size_t)k * P + i];
      if (stats) stats->pairs++;
      if (r.status != ORBM_FUSE_CANDIDATES) continue;                 // one of the `continue`s :1455-1509, or bestDist stayed 256
      int bestDist = r.best_dist, bestIdx = r.best_idx;
      const auto dMP = pMP->GetDescriptor();
      const uint8_t* d = dropin::mat_u8(dMP, 0);
      if (std::memcmp(d, &pts.desc[(size_t)32 * i], 32) != 0) {       // the descriptor is no longer the one the launch saw
        if (r.n_cand > ORBG_FUSE_CAND_CAP) {
          orbm_worldpoints_view one = pts.view;
          one.m = 1; one.pos += 3 * i; one.normal += 3 * i; one.min_dist += i; one.max_dist += i; one.desc = d;
          orbm_fuse_params prm{};
          prm.struct_size = sizeof(prm); prm.th = th; prm.sim3_form = 0;
          orbm_fuse_record r1;
          uint16_t c1[ORBG_FUSE_CAND_CAP];
          check(orbm_fuse(&kfs[k], 1, &one, nullptr, &prm, &r1, c1), "orbm_fuse");
          bestDist = r1.best_dist; bestIdx = r1.best_idx;
          if (stats) stats->relaunched++;
        } else {
          bestDist = 256; bestIdx = -1;
          const uint16_t* c = &cand[((size_t)k * P + i) * ORBG_FUSE_CAND_CAP];
          for (int j = 0; j < r.n_cand; j++) {
            const int dist = hamming256(d, dropin::mat_u8(pKF->mDescriptors, c[j]));
            if (dist < bestDist) { bestDist = dist; bestIdx = c[j]; }
          }
          if (stats) stats->rescored++;
        }
      }
      // If there is already a MapPoint replace otherwise add new measurement
      if (bestDist <= TH_LOW) {
        MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
          if (!pMPinKF->isBad()) {
            if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
            else pMPinKF->Replace(pMP);
          }
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
      }
    }
    return nFused;
  }
};

}  // namespace localmapping

// The body of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false).  Returns nFused, or -1 when pKF is out of scope (nothing has
// been changed: run the reference's body).
template <class KeyFrameT, class MapPointT>
int Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th, KeyFramesOnDevice<KeyFrameT>& onDevice, FuseStats* stats = nullptr) {
  if (!localmapping::in_scope(pKF)) return -1;
  localmapping::FuseLaunch<KeyFrameT, MapPointT> L(std::vector<KeyFrameT*>{pKF}, vpMapPoints, th, onDevice);
  return L.Replay(0, pKF, vpMapPoints, stats);
}

// The body of LocalMapping::SearchInNeighbors.  mbMonocular / mbInertial: the LocalMapping members; mbAbortBA: bool(), read where
// the reference reads the member (:898, :930).  Returns the number of target keyframes, or -1 when a keyframe is out of scope (nothing
// has been changed, no mnFuseTargetForKF mark written: run the reference's body).
template <class KeyFrameT, class AbortFn>
int SearchInNeighbors(KeyFrameT* mpCurrentKeyFrame, KeyFramesOnDevice<KeyFrameT>& onDevice, bool mbMonocular, bool mbInertial, AbortFn mbAbortBA,
                      FuseStats* stats = nullptr) {
  using MapPointT = typename std::remove_pointer<decltype(mpCurrentKeyFrame->GetMapPoint(0))>::type;
  // Retrieve neighbor keyframes (:871-917).  The marks are written after the scope check; until then `marked` stands for
  // "mnFuseTargetForKF == mpCurrentKeyFrame->mnId" of the keyframes this call has taken.
  int nn = 10;
  if (mbMonocular) nn = 20;
  const std::vector<KeyFrameT*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  std::vector<KeyFrameT*> vpTargetKFs;
  std::unordered_set<KeyFrameT*> marked;
  auto is_marked = [&](KeyFrameT* pKFi) { return marked.count(pKFi) || pKFi->mnFuseTargetForKF == mpCurrentKeyFrame->mnId; };
  for (KeyFrameT* pKFi : vpNeighKFs) {
    if (pKFi->isBad() || is_marked(pKFi)) continue;
    vpTargetKFs.push_back(pKFi);
    marked.insert(pKFi);
  }
  // Add some covisible of covisible; extend to some second neighbors if abort is not requested
  for (int i = 0, imax = (int)vpTargetKFs.size(); i < imax; i++) {
    const std::vector<KeyFrameT*> vpSecondNeighKFs = vpTargetKFs[i]->GetBestCovisibilityKeyFrames(20);
    for (KeyFrameT* pKFi2 : vpSecondNeighKFs) {
      if (pKFi2->isBad() || is_marked(pKFi2) || pKFi2->mnId == mpCurrentKeyFrame->mnId) continue;
      vpTargetKFs.push_back(pKFi2);
      marked.insert(pKFi2);
    }
    if (mbAbortBA()) break;
  }
  // Extend to temporal neighbors
  if (mbInertial) {
    KeyFrameT* pKFi = mpCurrentKeyFrame->mPrevKF;
    while (vpTargetKFs.size() < 20 && pKFi) {
      if (pKFi->isBad() || is_marked(pKFi)) { pKFi = pKFi->mPrevKF; continue; }
      vpTargetKFs.push_back(pKFi);
      marked.insert(pKFi);
      pKFi = pKFi->mPrevKF;
    }
  }
  if (!localmapping::in_scope(mpCurrentKeyFrame) || (int)vpTargetKFs.size() > ORBG_FUSE_MAX_KEYFRAMES) return -1;
  for (KeyFrameT* pKFi : vpTargetKFs)
    if (!localmapping::in_scope(pKFi)) return -1;
  for (KeyFrameT* pKFi : vpTargetKFs) pKFi->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;

  // Search matches by projection from current KF in target KFs: one launch, then the replay target by target
  const float th = 3.0f;                                                            // Fuse's default, I/ORBmatcher.h
  std::vector<MapPointT*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  {
    localmapping::FuseLaunch<KeyFrameT, MapPointT> L(vpTargetKFs, vpMapPointMatches, th, onDevice);
    for (size_t k = 0; k < vpTargetKFs.size(); k++) L.Replay((int)k, vpTargetKFs[k], vpMapPointMatches, stats);
  }
  if (mbAbortBA()) return (int)vpTargetKFs.size();

  // Search matches by projection from target KFs in current KF
  std::vector<MapPointT*> vpFuseCandidates;
  vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
  for (KeyFrameT* pKFi : vpTargetKFs) {
    std::vector<MapPointT*> vpMapPointsKFi = pKFi->GetMapPointMatches();
    for (MapPointT* pMP : vpMapPointsKFi) {
      if (!pMP) continue;
      if (pMP->isBad() || pMP->mnFuseCandidateForKF == mpCurrentKeyFrame->mnId) continue;
      pMP->mnFuseCandidateForKF = mpCurrentKeyFrame->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }
  Fuse(mpCurrentKeyFrame, vpFuseCandidates, th, onDevice, stats);

  // Update points
  vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
    MapPointT* pMP = vpMapPointMatches[i];
    if (pMP) {
      if (!pMP->isBad()) {
        pMP->ComputeDistinctiveDescriptors();
        pMP->UpdateNormalAndDepth();
      }
    }
  }
  // Update connections in covisibility graph
  mpCurrentKeyFrame->UpdateConnections();
  return (int)vpTargetKFs.size();
}

}  // namespace orbgpu

#endif  // ORBGPU_LOCALMAPPING_HPP_
