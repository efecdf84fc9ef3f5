// Stand-ins for the members of Frame / MapPoint / GeometricCamera that MLPnPsolver's constructor reads (S/MLPnPsolver.cpp:54-96) and
// that tests/cpp/mock_orbslam3.hpp does not carry: Frame::mvLevelSigma2 and the camera's unproject.  The types are independent of the
// mocks there (they share its Mat, KeyPoint and GeometricCamera).  Every member the glue may touch is public in the reference; under
// -DMOCK_STRICT_ACCESS what the reference keeps protected is protected here, and scenes are set up through the Test* members.
#pragma once
#include <vector>

#include "mock_orbslam3.hpp"

namespace mock_mlpnp {

using mock::KeyPoint;
using mock::Mat;
using mock::Point2f;

struct Point3f { float x, y, z; };

// Pinhole (S/CameraModels/Pinhole.cpp:59-62): unproject in float
class Camera : public mock::GeometricCamera {
 public:
  Camera(unsigned type, std::vector<float> params) : mock::GeometricCamera(type, std::move(params)) {}
  Point3f unproject(const Point2f& p2D) {                                             // ref: I/CameraModels/GeometricCamera.h unproject
    return Point3f{(p2D.x - mvParameters[2]) / mvParameters[0], (p2D.y - mvParameters[3]) / mvParameters[1], 1.f};
  }
};

class MapPoint {
 public:
  Mat GetWorldPos() const { return mWorldPos; }                                       // ref: I/MapPoint.h GetWorldPos
  bool isBad() const { return mbBad; }                                                // ref: I/MapPoint.h isBad
 MOCK_PROTECTED:
  Mat mWorldPos{3, 1, 4};
  bool mbBad = false;
 public:      // ---- test instrumentation
  void TestSetWorldPos(float x, float y, float z) { float* p = mWorldPos.ptr<float>(0); p[0] = x; p[1] = y; p[2] = z; }
  void TestSetBad(bool b) { mbBad = b; }
};

class Frame {
 public:
  std::vector<KeyPoint> mvKeysUn;                                                     // ref: I/Frame.h mvKeysUn
  std::vector<float> mvLevelSigma2;                                                   // ref: I/Frame.h mvLevelSigma2
  std::vector<MapPoint*> mvpMapPoints;                                                // ref: I/Frame.h mvpMapPoints
  Camera* mpCamera = nullptr;                                                         // ref: I/Frame.h mpCamera
  void TestSetLevels(int n_levels, float scale_factor) {                              // ORBextractor's tables, S/ORBextractor.cc:413-423
    mvLevelSigma2.assign(n_levels, 1.0f);
    float sf = 1.0f;
    for (int i = 1; i < n_levels; i++) { sf = sf * scale_factor; mvLevelSigma2[i] = sf * sf; }
  }
};

}  // namespace mock_mlpnp
