// Stand-ins for the members of KeyFrame / MapPoint that Sim3Solver's constructor reads (S/Sim3Solver.cc:38-128) and that
// tests/cpp/mock_orbslam3.hpp does not carry: GetIndexInKeyFrame, GetRotation, GetTranslation and a keyframe's mvLevelSigma2.  The
// types are independent of the mocks there (they share its Mat, KeyPoint and GeometricCamera).  Every member the glue may touch is
// public in the reference; its line there is named in the `// ref:` note of its declaration, and tests/test_sim3_cpu.py holds those
// notes against the reference's headers where they are present.  Under -DMOCK_STRICT_ACCESS what the reference keeps protected is
// protected here, and scenes are set up through the Test* members (no counterpart in the reference; the glue never names them).
#pragma once
#include <map>
#include <tuple>
#include <vector>

#include "mock_orbslam3.hpp"

namespace mock_sim3 {

using mock::GeometricCamera;
using mock::KeyPoint;
using mock::Mat;

class KeyFrame;

class MapPoint {
 public:
  Mat GetWorldPos() const { return mWorldPos; }                                      // ref: I/MapPoint.h:128 GetWorldPos
  bool isBad() const { return mbBad; }                                                // ref: I/MapPoint.h:143 isBad
  std::tuple<int, int> GetIndexInKeyFrame(KeyFrame* pKF) const {                      // ref: I/MapPoint.h:139 GetIndexInKeyFrame
    const auto it = mObservations.find(pKF);                                          // S/MapPoint.cc: (-1, -1) when pKF does not observe the point
    return it == mObservations.end() ? std::make_tuple(-1, -1) : it->second;
  }
 MOCK_PROTECTED:
  Mat mWorldPos{3, 1, 4};
  std::map<KeyFrame*, std::tuple<int, int>> mObservations;
  bool mbBad = false;
 public:      // ---- test instrumentation
  void TestSetWorldPos(float x, float y, float z) { float* p = mWorldPos.ptr<float>(0); p[0] = x; p[1] = y; p[2] = z; }
  void TestSetBad(bool b) { mbBad = b; }
  void TestObserve(KeyFrame* kf, int idx) { mObservations[kf] = std::make_tuple(idx, -1); }
};

class KeyFrame {
 public:
  Mat GetRotation() const {                                                           // ref: I/KeyFrame.h:286 GetRotation
    Mat R(3, 3, 4);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.ptr<float>(i)[j] = Tcw.at(i, j);
    return R;
  }
  Mat GetTranslation() const {                                                        // ref: I/KeyFrame.h:288 GetTranslation
    Mat t(3, 1, 4);
    for (int i = 0; i < 3; i++) t.ptr<float>(i)[0] = Tcw.at(i, 3);
    return t;
  }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }          // ref: I/KeyFrame.h:330 GetMapPointMatches
  std::vector<KeyPoint> mvKeysUn;                                                     // ref: I/KeyFrame.h:478 mvKeysUn
  std::vector<float> mvLevelSigma2;                                                   // ref: I/KeyFrame.h:497 mvLevelSigma2
  GeometricCamera* mpCamera = nullptr;                                                // ref: I/KeyFrame.h:635 mpCamera
 MOCK_PROTECTED:
  std::vector<MapPoint*> mvpMapPoints;
  Mat Tcw{4, 4, 4};
 public:      // ---- test instrumentation
  void TestSetPose(const float* T16) { for (int i = 0; i < 16; i++) Tcw.ptr<float>(0)[i] = T16[i]; }
  void TestSetMapPoints(const std::vector<MapPoint*>& v) { mvpMapPoints = v; }
  void TestSetLevels(int n_levels, float scale_factor) {                              // ORBextractor's tables, S/ORBextractor.cc:413-423
    mvLevelSigma2.assign(n_levels, 1.0f);
    float sf = 1.0f;
    for (int i = 1; i < n_levels; i++) { sf = sf * scale_factor; mvLevelSigma2[i] = sf * sf; }
  }
};

}  // namespace mock_sim3
