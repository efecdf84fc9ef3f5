// Stand-ins for what Optimizer::OptimizeSim3 (S/Optimizer.cc:4031-4310) reads and that mock_sim3.hpp does not carry: a keyframe's
// mvInvLevelSigma2, a map point's mnTrackScaleLevel, and a minimal g2o::Sim3 with the quaternion / vector types it is built from (no
// Eigen here).  Same rules as mock_sim3.hpp: every member the glue may touch is public in the reference and names its line in a
// `// ref:` note (I/: the reference's include directory, G/: Thirdparty/g2o/g2o), which tests/test_sim3_opt_cpu.py holds against
// the reference's headers where they are present; scenes are set up through the Test* members.
#pragma once
#include <vector>

#include "mock_sim3.hpp"

namespace mock_sim3_opt {

class MapPoint : public mock_sim3::MapPoint {
 public:
  int mnTrackScaleLevel = 0;                                                          // ref: I/MapPoint.h:212 mnTrackScaleLevel
};

class KeyFrame : public mock_sim3::KeyFrame {
 public:
  std::vector<float> mvInvLevelSigma2;                                                // ref: I/KeyFrame.h:498 mvInvLevelSigma2
  void TestSetInvLevels(int n_levels, float scale_factor) {                           // ORBextractor's tables, S/ORBextractor.cc:413-423
    TestSetLevels(n_levels, scale_factor);
    mvInvLevelSigma2.resize(n_levels);
    for (int i = 0; i < n_levels; i++) mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i];
  }
};

// Eigen::Vector3d / Eigen::Quaterniond as far as g2o::Sim3's users need them
struct Vector3d {
  double v[3];
  Vector3d(double x, double y, double z) : v{x, y, z} {}
  double operator[](int i) const { return v[i]; }
};
struct QuatCoeffs {
  double c[4];                                                                        // x, y, z, w: Eigen's storage order
  double operator[](int i) const { return c[i]; }
};
struct Quaterniond {
  QuatCoeffs c;
  Quaterniond(double w, double x, double y, double z) : c{{x, y, z, w}} {}            // Eigen's constructor order
  const QuatCoeffs& coeffs() const { return c; }
};

class Sim3 {
 public:
  Sim3(const Quaterniond& r, const Vector3d& t, double s) : r(r), t(t), s(s) {}       // ref: G/types/sim3.h:59 Sim3
  const Vector3d& translation() const { return t; }                                   // ref: G/types/sim3.h:280 translation
  const Quaterniond& rotation() const { return r; }                                   // ref: G/types/sim3.h:284 rotation
  const double& scale() const { return s; }                                           // ref: G/types/sim3.h:288 scale
 protected:
  Quaterniond r;
  Vector3d t;
  double s;
};

struct Matrix7d {                                                                     // Eigen::Matrix<double, 7, 7>
  double m[49];
  double& operator()(int i, int j) { return m[7 * i + j]; }
};

}  // namespace mock_sim3_opt
