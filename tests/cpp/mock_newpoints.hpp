// Stand-ins for the members of KeyFrame / MapPoint that LocalMapping::CreateNewMapPoints and ORBmatcher::SearchForTriangulation read
// or write (S/LocalMapping.cc:520-865, S/ORBmatcher.cc:961-1202) and that tests/cpp/mock_orbslam3.hpp does not carry.  The types are
// independent of the mocks there (they share its Mat, KeyPoint, FeatureVector and GeometricCamera).  Every member the glue
// (include/orbgpu_localmapping.hpp) touches is public in the reference; its line in I/KeyFrame.h / I/MapPoint.h is named in the
// `// ref:` note of its declaration.  Under -DMOCK_STRICT_ACCESS what the reference keeps protected is protected here, and scenes are
// set up through the Test* members (no counterpart in the reference; the glue never names them).
#pragma once
#include <map>
#include <vector>

#include "mock_orbslam3.hpp"

namespace mock_np {

using mock::FeatureVector;
using mock::GeometricCamera;
using mock::KeyPoint;
using mock::Mat;

class KeyFrame;

class MapPoint {
 public:
  MapPoint(const Mat& Pos, KeyFrame* pRefKF) : mWorldPos(Pos), mpRefKF(pRefKF) {}             // ref: I/MapPoint.h:121 MapPoint(Pos, pRefKF, ...)
  Mat GetWorldPos() const { return mWorldPos; }                                              // ref: I/MapPoint.h:128 GetWorldPos
  void AddObservation(KeyFrame* pKF, int idx) { mObservations[pKF] = idx; }                   // ref: I/MapPoint.h:136 AddObservation
  void ComputeDistinctiveDescriptors() { n_distinctive++; }                                  // ref: I/MapPoint.h:155 ComputeDistinctiveDescriptors
  void UpdateNormalAndDepth() { n_normal_updates++; }                                        // ref: I/MapPoint.h:159 UpdateNormalAndDepth
 MOCK_PROTECTED:
  Mat mWorldPos{3, 1, 4};
  KeyFrame* mpRefKF = nullptr;
  std::map<KeyFrame*, int> mObservations;
 public:      // ---- test instrumentation
  int n_distinctive = 0, n_normal_updates = 0;
  const std::map<KeyFrame*, int>& TestObservations() const { return mObservations; }
  KeyFrame* TestRefKF() const { return mpRefKF; }
};

class KeyFrame {
 public:
  Mat GetPose() const { return Tcw; }                                                         // ref: I/KeyFrame.h:279 GetPose
  Mat GetPoseInverse() const { return Twc; }                                                  // ref: I/KeyFrame.h:280 GetPoseInverse
  Mat GetCameraCenter() const { return Ow; }                                                  // ref: I/KeyFrame.h:281 GetCameraCenter
  Mat GetRotation() const {                                                                   // ref: I/KeyFrame.h:286 GetRotation
    Mat R(3, 3, 4);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.ptr<float>(i)[j] = Tcw.at(i, j);
    return R;
  }
  Mat GetTranslation() const {                                                                // ref: I/KeyFrame.h:288 GetTranslation
    Mat t(3, 1, 4);
    for (int i = 0; i < 3; i++) t.ptr<float>(i)[0] = Tcw.at(i, 3);
    return t;
  }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {                         // ref: I/KeyFrame.h:302 GetBestCovisibilityKeyFrames
    if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
  }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }              // ref: I/KeyFrame.h:325 AddMapPoint
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }                  // ref: I/KeyFrame.h:330 GetMapPointMatches
  MapPoint* GetMapPoint(const size_t& idx) const { return mvpMapPoints[idx]; }                // ref: I/KeyFrame.h:332 GetMapPoint
  float ComputeSceneMedianDepth(const int /*q*/) { return test_median_depth; }                // ref: I/KeyFrame.h:350 ComputeSceneMedianDepth
  float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0;                // ref: I/KeyFrame.h:470 fx
  int N = 0;                                                                                  // ref: I/KeyFrame.h:474 N
  std::vector<KeyPoint> mvKeys;                                                               // ref: I/KeyFrame.h:477 mvKeys
  std::vector<KeyPoint> mvKeysUn;                                                             // ref: I/KeyFrame.h:478 mvKeysUn
  std::vector<float> mvuRight;                                                                // ref: I/KeyFrame.h:479 mvuRight
  std::vector<float> mvDepth;                                                                 // ref: I/KeyFrame.h:482 mvDepth
  Mat mDescriptors;                                                                           // ref: I/KeyFrame.h:483 mDescriptors
  FeatureVector mFeatVec;                                                                     // ref: I/KeyFrame.h:487 mFeatVec
  int mnScaleLevels = 8;                                                                      // ref: I/KeyFrame.h:493 mnScaleLevels
  float mfScaleFactor = 1.2f;                                                                 // ref: I/KeyFrame.h:494 mfScaleFactor
  std::vector<float> mvScaleFactors;                                                          // ref: I/KeyFrame.h:496 mvScaleFactors
  std::vector<float> mvLevelSigma2;                                                           // ref: I/KeyFrame.h:497 mvLevelSigma2
  int mnMinX = 0, mnMinY = 0, mnMaxX = 752, mnMaxY = 480;                                     // ref: I/KeyFrame.h:501 mnMinX
  KeyFrame* mPrevKF = nullptr;                                                                // ref: I/KeyFrame.h:508 mPrevKF
  GeometricCamera* mpCamera = nullptr; GeometricCamera* mpCamera2 = nullptr;                  // ref: I/KeyFrame.h:635 mpCamera
  int NLeft = -1, NRight = -1;                                                                // ref: I/KeyFrame.h:648 NLeft
 MOCK_PROTECTED:
  Mat Tcw{4, 4, 4}, Twc{4, 4, 4}, Ow{3, 1, 4};
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
 public:      // ---- test instrumentation
  float test_median_depth = 5.f;
  // KeyFrame::SetPose, S/KeyFrame.cc:139-160: Rwc = Rcw.t(), Ow = -Rwc * tcw (cv::gemm: double accumulation, one rounding), Twc = [Rwc | Ow]
  void TestSetPose(const float* T12) {
    float* T = Tcw.ptr<float>(0); float* W = Twc.ptr<float>(0); float* O = Ow.ptr<float>(0);
    for (int i = 0; i < 12; i++) T[i] = T12[i];
    T[12] = T[13] = T[14] = 0; T[15] = 1;
    for (int i = 0; i < 3; i++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += (double)T[4 * k + i] * (double)T[4 * k + 3];
      O[i] = (float)(-s);
      for (int j = 0; j < 3; j++) W[4 * i + j] = T[4 * j + i];
      W[4 * i + 3] = O[i];
    }
    W[12] = W[13] = W[14] = 0; W[15] = 1;
  }
  void TestSetLevels(int n_levels, float scale_factor) {                                      // ORBextractor's tables, S/ORBextractor.cc:413-423
    mnScaleLevels = n_levels; mfScaleFactor = scale_factor;
    mvScaleFactors.assign(n_levels, 1.0f); mvLevelSigma2.assign(n_levels, 1.0f);
    for (int i = 1; i < n_levels; i++) { mvScaleFactors[i] = mvScaleFactors[i - 1] * scale_factor; mvLevelSigma2[i] = mvScaleFactors[i] * mvScaleFactors[i]; }
  }
  void TestSetMapPoints(const std::vector<MapPoint*>& v) { mvpMapPoints = v; }
  void TestSetNeighbours(const std::vector<KeyFrame*>& v) { mvpOrderedConnectedKeyFrames = v; }
};

}  // namespace mock_np
