// Stand-ins for the members of KeyFrame / MapPoint that LocalMapping::SearchInNeighbors and ORBmatcher::Fuse read or write
// (S/LocalMapping.cc:868-976, S/ORBmatcher.cc:1395-1605, S/MapPoint.cc:231-264, 367-419).  The types are independent of the other
// mocks (they share mock_orbslam3.hpp's Mat, KeyPoint and GeometricCamera).  Every member the glue (include/orbgpu_localmapping.hpp)
// touches is public in the reference; its line in I/KeyFrame.h / I/MapPoint.h is named in the `// ref:` note of its declaration.
// The exception is the raw distance range, which the reference keeps protected: GetMinDistance() / GetMaxDistance() are edit E1 of
// INTEGRATION.md, which the Tracking glue needs already.  Under -DMOCK_STRICT_ACCESS what the reference keeps protected is protected
// here, and scenes are set up through the Test* members (no counterpart in the reference; the glue never names them).
// Replace, AddObservation and IsInKeyFrame follow S/MapPoint.cc statement by statement (a stereo observation counts twice);
// ComputeDistinctiveDescriptors really changes the descriptor (to that of the median observation in keyframe-id order), so that a
// point met again after a Replace carries other bytes than the launch saw.
#pragma once
#include <map>
#include <set>
#include <vector>

#include "mock_orbslam3.hpp"

namespace mock_fuse {

using mock::GeometricCamera;
using mock::KeyPoint;
using mock::Mat;

class MapPoint;

class KeyFrame {
 public:
  long unsigned int mnId = 0;                                                                 // ref: I/KeyFrame.h:404 mnId
  long unsigned int mnFuseTargetForKF = 0;                                                    // ref: I/KeyFrame.h:421 mnFuseTargetForKF
  Mat GetPose() const { return Tcw; }                                                         // ref: I/KeyFrame.h:279 GetPose
  Mat GetCameraCenter() const { return Ow; }                                                  // ref: I/KeyFrame.h:281 GetCameraCenter
  void UpdateConnections(bool = true) { n_update_connections++; }                             // ref: I/KeyFrame.h:298 UpdateConnections
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {                         // ref: I/KeyFrame.h:302 GetBestCovisibilityKeyFrames
    if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
  }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }              // ref: I/KeyFrame.h:325 AddMapPoint
  void EraseMapPointMatch(const int& idx) { mvpMapPoints[idx] = nullptr; }
  void ReplaceMapPointMatch(const int& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }                  // ref: I/KeyFrame.h:330 GetMapPointMatches
  MapPoint* GetMapPoint(const size_t& idx) const { return mvpMapPoints[idx]; }                // ref: I/KeyFrame.h:332 GetMapPoint
  bool isBad() const { return mbBad; }                                                        // ref: I/KeyFrame.h:347 isBad
  float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0;                // ref: I/KeyFrame.h:470 fx
  int N = 0;                                                                                  // ref: I/KeyFrame.h:474 N
  std::vector<KeyPoint> mvKeysUn;                                                             // ref: I/KeyFrame.h:478 mvKeysUn
  std::vector<float> mvuRight;                                                                // ref: I/KeyFrame.h:481 mvuRight
  std::vector<float> mvDepth;                                                                 // ref: I/KeyFrame.h:482 mvDepth
  Mat mDescriptors;                                                                           // ref: I/KeyFrame.h:483 mDescriptors
  int mnScaleLevels = 8;                                                                      // ref: I/KeyFrame.h:493 mnScaleLevels
  float mfScaleFactor = 1.2f;                                                                 // ref: I/KeyFrame.h:494 mfScaleFactor
  float mfLogScaleFactor = 0.f;                                                               // ref: I/KeyFrame.h:495 mfLogScaleFactor
  std::vector<float> mvScaleFactors;                                                          // ref: I/KeyFrame.h:496 mvScaleFactors
  std::vector<float> mvInvLevelSigma2;                                                        // ref: I/KeyFrame.h:498 mvInvLevelSigma2
  int mnMinX = 0, mnMinY = 0, mnMaxX = 752, mnMaxY = 480;                                     // ref: I/KeyFrame.h:501 mnMinX
  KeyFrame* mPrevKF = nullptr;                                                                // ref: I/KeyFrame.h:508 mPrevKF
  GeometricCamera* mpCamera = nullptr; GeometricCamera* mpCamera2 = nullptr;                  // ref: I/KeyFrame.h:635 mpCamera
  int NLeft = -1, NRight = -1;                                                                // ref: I/KeyFrame.h:648 NLeft
 MOCK_PROTECTED:
  Mat Tcw{4, 4, 4}, Ow{3, 1, 4};
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  bool mbBad = false;
 public:      // ---- test instrumentation
  int n_update_connections = 0;
  // KeyFrame::SetPose, S/KeyFrame.cc:139-160: Ow = -Rcw.t() * tcw (cv::gemm: double accumulation, one rounding)
  void TestSetPose(const float* T12) {
    float* T = Tcw.ptr<float>(0); float* O = Ow.ptr<float>(0);
    for (int i = 0; i < 12; i++) T[i] = T12[i];
    T[12] = T[13] = T[14] = 0; T[15] = 1;
    for (int i = 0; i < 3; i++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += (double)T[4 * k + i] * (double)T[4 * k + 3];
      O[i] = (float)(-s);
    }
  }
  void TestSetLevels(int n_levels, float scale_factor) {                                      // ORBextractor's tables, S/ORBextractor.cc:413-423
    mnScaleLevels = n_levels; mfScaleFactor = scale_factor; mfLogScaleFactor = std::log(scale_factor);
    mvScaleFactors.assign(n_levels, 1.0f); mvInvLevelSigma2.assign(n_levels, 1.0f);
    for (int i = 1; i < n_levels; i++) {
      mvScaleFactors[i] = mvScaleFactors[i - 1] * scale_factor;
      mvInvLevelSigma2[i] = 1.0f / (mvScaleFactors[i] * mvScaleFactors[i]);
    }
  }
  void TestSetMapPoints(const std::vector<MapPoint*>& v) { mvpMapPoints = v; }
  void TestSetNeighbours(const std::vector<KeyFrame*>& v) { mvpOrderedConnectedKeyFrames = v; }
  void TestSetBad() { mbBad = true; }
  const Mat& TestTcw() const { return Tcw; }
  // KeyFrame::GetFeaturesInArea's grid (S/Frame.cc:360-391 through the KeyFrame constructor), for the serial restatement
  std::vector<std::vector<std::vector<size_t>>> test_grid;
  float test_w_inv = 0, test_h_inv = 0;
  void TestBuildGrid() {
    test_w_inv = 64.f / (float)(mnMaxX - mnMinX); test_h_inv = 48.f / (float)(mnMaxY - mnMinY);
    test_grid.assign(64, std::vector<std::vector<size_t>>(48));
    for (int i = 0; i < N; i++) {
      const int px = (int)std::round((mvKeysUn[i].pt.x - mnMinX) * test_w_inv), py = (int)std::round((mvKeysUn[i].pt.y - mnMinY) * test_h_inv);
      if (px < 0 || px >= 64 || py < 0 || py >= 48) continue;
      test_grid[px][py].push_back((size_t)i);
    }
  }
};

class MapPoint {
 public:
  MapPoint(long unsigned id, const float* X, const float* normal, float min_d, float max_d, const uint8_t* desc) : mnId(id), mfMinDistance(min_d), mfMaxDistance(max_d) {
    for (int i = 0; i < 3; i++) { mWorldPos.ptr<float>(i)[0] = X[i]; mNormalVector.ptr<float>(i)[0] = normal[i]; }
    std::memcpy(mDescriptor.ptr<uint8_t>(0), desc, 32);
  }
  long unsigned int mnId = 0;
  long unsigned int mnFuseCandidateForKF = 0;                                                 // ref: I/MapPoint.h:219 mnFuseCandidateForKF
  Mat GetWorldPos() const { return mWorldPos; }                                               // ref: I/MapPoint.h:128 GetWorldPos
  Mat GetNormal() const { return mNormalVector; }                                             // ref: I/MapPoint.h:130 GetNormal
  int Observations() const { return nObs; }                                                   // ref: I/MapPoint.h:134 Observations
  void AddObservation(KeyFrame* pKF, int idx) {                                               // ref: I/MapPoint.h:136 AddObservation
    mObservations[pKF] = idx;                       // S/MapPoint.cc:231-264 (NLeft == -1: the left index is overwritten, nObs grows either way)
    if (!pKF->mpCamera2 && pKF->mvuRight[idx] >= 0) nObs += 2; else nObs++;
  }
  bool IsInKeyFrame(KeyFrame* pKF) const { return mObservations.count(pKF) != 0; }            // ref: I/MapPoint.h:140 IsInKeyFrame
  bool isBad() const { return mbBad; }                                                        // ref: I/MapPoint.h:143 isBad
  void Replace(MapPoint* pMP) {                                                               // ref: I/MapPoint.h:145 Replace
    if (pMP->mnId == this->mnId) return;
    std::map<KeyFrame*, int, ById> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    mpReplaced = pMP;
    for (auto& ob : obs) {
      KeyFrame* pKF = ob.first;
      if (!pMP->IsInKeyFrame(pKF)) { pKF->ReplaceMapPointMatch(ob.second, pMP); pMP->AddObservation(pKF, ob.second); }
      else pKF->EraseMapPointMatch(ob.second);
    }
    pMP->ComputeDistinctiveDescriptors();
  }
  void ComputeDistinctiveDescriptors() {                                                      // ref: I/MapPoint.h:155 ComputeDistinctiveDescriptors
    n_distinctive++;
    if (mObservations.empty()) return;
    auto it = mObservations.begin();
    std::advance(it, (mObservations.size() - 1) / 2);
    std::memcpy(mDescriptor.ptr<uint8_t>(0), it->first->mDescriptors.ptr<uint8_t>(it->second), 32);
  }
  Mat GetDescriptor() const { return mDescriptor; }                                           // ref: I/MapPoint.h:157 GetDescriptor
  void UpdateNormalAndDepth() { n_normal_updates++; }                                         // ref: I/MapPoint.h:159 UpdateNormalAndDepth
  float GetMinDistance() const { return mfMinDistance; }                                      // INTEGRATION.md edit E1
  float GetMaxDistance() const { return mfMaxDistance; }                                      // INTEGRATION.md edit E1
  float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
 MOCK_PROTECTED:
  struct ById { bool operator()(const KeyFrame* a, const KeyFrame* b) const { return a->mnId < b->mnId; } };   // (the same order in both copies of a map)
  float mfMinDistance = 0, mfMaxDistance = 0;
  Mat mWorldPos{3, 1, 4}, mNormalVector{3, 1, 4}, mDescriptor{1, 32, 1};
  std::map<KeyFrame*, int, ById> mObservations;
  bool mbBad = false;
  MapPoint* mpReplaced = nullptr;
  int nObs = 0;
 public:      // ---- test instrumentation
  int n_distinctive = 0, n_normal_updates = 0;
  const std::map<KeyFrame*, int, ById>& TestObservations() const { return mObservations; }
  MapPoint* TestReplaced() const { return mpReplaced; }
  float TestMaxDistance() const { return mfMaxDistance; }
};

}  // namespace mock_fuse
