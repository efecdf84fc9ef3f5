// Minimal stand-ins for what orbgpu::InertialOptimization (orbgpu_inertial.hpp) reads and writes beyond tests/cpp/mock_inertial_ba.hpp: a
// Map with GetMaxKFid / GetAllKeyFrames, a KeyFrame whose predecessor and map are of these types, a preintegration that can Reintegrate,
// and the two Eigen types the reference's signatures name (element access through operator() is all the glue uses).  Mat, Bias and the
// event log are mock_inertial_ba.hpp's.
#pragma once

#include <vector>

#include "mock_inertial_ba.hpp"

namespace mocki {

using mock::Bias;
using mock::Mat;
using mock::log;

struct Matrix3d {
  double d[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double& operator()(int i, int j) { return d[3 * i + j]; }
  double operator()(int i, int j) const { return d[3 * i + j]; }
};
struct Vector3d {
  double d[3] = {0, 0, 0};
  double& operator()(int i) { return d[i]; }
  double operator()(int i) const { return d[i]; }
};
struct MatrixXd { int touched = 0; };        // covInertial: the glue must not look at it

struct Preintegrated : mock::Preintegrated {
  void Reintegrate() { log("Reintegrate " + std::to_string(owner)); }
};

class KeyFrame;
class Map {
 public:
  unsigned long max_id = 0;
  std::vector<KeyFrame*> all;
  unsigned long GetMaxKFid() const { return max_id; }
  std::vector<KeyFrame*> GetAllKeyFrames() const { return all; }
};

class KeyFrame {
 public:
  unsigned long mnId = 0;
  KeyFrame* mPrevKF = nullptr;
  bool bad = false;
  Preintegrated* mpImuPreintegrated = nullptr;
  Map* map = nullptr;
  Map* GetMap() const { return map; }
  bool isBad() const { return bad; }
  Mat GetImuRotation() const { return R; }
  Mat GetImuPosition() const { return t; }
  Mat GetVelocity() const { return v; }
  Mat GetGyroBias() const { Mat m(3, 1); m.d = {bias.bwx, bias.bwy, bias.bwz}; return m; }
  Mat GetAccBias() const { Mat m(3, 1); m.d = {bias.bax, bias.bay, bias.baz}; return m; }
  Bias GetImuBias() const { return bias; }
  void SetVelocity(const Mat& m) { v = m; log("SetVelocity " + std::to_string(mnId) + " " + std::to_string(m.d[0])); }
  void SetNewBias(const Bias& b) { bias = b; log("SetNewBias " + std::to_string(mnId) + " " + std::to_string(b.bwx) + " " + std::to_string(b.bax)); }
#ifdef MOCK_STRICT_ACCESS
 private:
  friend struct Access;
#endif
  Mat R{3, 3}, t{3, 1}, v{3, 1};
  Bias bias;
};

struct Access {
  static Mat& R(KeyFrame& k) { return k.R; }
  static Mat& t(KeyFrame& k) { return k.t; }
  static Mat& v(KeyFrame& k) { return k.v; }
  static Bias& bias(KeyFrame& k) { return k.bias; }
};

}  // namespace mocki
