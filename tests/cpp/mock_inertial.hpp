// Minimal stand-ins for the reference's types that orbgpu_inertial.hpp reads and writes (Frame, KeyFrame, MapPoint, IMU::Bias,
// IMU::Calib, IMU::Preintegrated, ConstraintPoseImu), for tests/cpp/pose_inertial_glue.cpp.  With -DMOCK_STRICT_ACCESS every member
// the reference keeps private or behind a getter is reachable only the way the reference allows.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace mock {

struct Mat {
  int rows = 0, cols = 0;
  std::vector<float> d;
  Mat() = default;
  Mat(int r, int c) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
};
inline const float* mat_f32(const Mat& m) { return m.d.data(); }
inline void make_mat(Mat& out, int rows, int cols, const float* data) { out = Mat(rows, cols); std::memcpy(out.d.data(), data, sizeof(float) * rows * cols); }

struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; int octave = 0; };

class MapPoint {
 public:
  float mTrackDepth = 0;
  explicit MapPoint(const float* X) : pos(3, 1) { std::memcpy(pos.d.data(), X, 12); }
  Mat GetWorldPos() const { return pos; }
#ifndef MOCK_STRICT_ACCESS
  Mat pos;
#else
 private:
  Mat pos;
#endif
};

struct Bias {
  float bax = 0, bay = 0, baz = 0, bwx = 0, bwy = 0, bwz = 0;
  Bias() = default;
  Bias(float ax, float ay, float az, float wx, float wy, float wz) : bax(ax), bay(ay), baz(az), bwx(wx), bwy(wy), bwz(wz) {}
};
struct Calib { Mat Tcb{4, 4}; };
struct Preintegrated {
  float dT = 0;
  Mat C{15, 15}, dR{3, 3}, dV{3, 1}, dP{3, 1}, JRg{3, 3}, JVg{3, 3}, JVa{3, 3}, JPg{3, 3}, JPa{3, 3};
  Bias b;
};

// Eigen-like fixed arrays: operator()(i) / operator()(i, j)
template <int N> struct Vec { double v[N] = {}; double operator()(int i) const { return v[i]; } };
template <int R, int C> struct Mtx { double v[R * C] = {}; double operator()(int i, int j) const { return v[i * C + j]; } };
struct ConstraintPoseImu {
  Mtx<3, 3> Rwb; Vec<3> twb, vwb, bg, ba; Mtx<15, 15> H;
  static int live;                                     // constructions minus destructions: the glue must not leak or double-free
  ConstraintPoseImu() { live++; }
  ~ConstraintPoseImu() { live--; }
};
inline int ConstraintPoseImu::live = 0;

class KeyFrame {
 public:
  Mat GetImuRotation() const { return R; }
  Mat GetImuPosition() const { return t; }
  Mat GetVelocity() const { return v; }
  Mat GetGyroBias() const { return bg; }
  Mat GetAccBias() const { return ba; }
  void set(const Mat& R_, const Mat& t_, const Mat& v_, const Mat& bg_, const Mat& ba_) { R = R_; t = t_; v = v_; bg = bg_; ba = ba_; }
#ifdef MOCK_STRICT_ACCESS
 private:
#endif
  Mat R{3, 3}, t{3, 1}, v{3, 1}, bg{3, 1}, ba{3, 1};
};

class Frame {
 public:
  int N = 0, Nleft = -1;
  void* mpCamera2 = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  Calib mImuCalib;
  Mat mVw{3, 1};
  Bias mImuBias;
  Preintegrated* mpImuPreintegrated = nullptr;
  Preintegrated* mpImuPreintegratedFrame = nullptr;
  KeyFrame* mpLastKeyFrame = nullptr;
  Frame* mpPrevFrame = nullptr;
  ConstraintPoseImu* mpcpi = nullptr;
  Mat GetImuRotation() const { return Rwb; }
  Mat GetImuPosition() const { return twb; }
  void SetImuPoseVelocity(const Mat& R, const Mat& t, const Mat& v) { Rwb = R; twb = t; mVw = v; set_calls++; }
  int set_calls = 0;
#ifdef MOCK_STRICT_ACCESS
 private:
#endif
  Mat Rwb{3, 3}, twb{3, 1};
};

}  // namespace mock
