// Minimal stand-ins for the reference's types that orbgpu::LocalInertialBA (orbgpu_inertial.hpp) reads and writes -- KeyFrame, MapPoint,
// Map, IMU::Bias, IMU::Calib, IMU::Preintegrated --, for tests/cpp/inertial_ba_glue.cpp.  Every call the reference makes with a visible
// effect is appended to an event log, so that the test can read the ORDER of the glue's writes.  With -DMOCK_STRICT_ACCESS what the
// reference keeps behind a getter is reachable only that way.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace mock {

inline std::vector<std::string>& events() { static std::vector<std::string> e; return e; }
inline void log(const std::string& s) { events().push_back(s); }

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

struct Bias {
  float bax = 0, bay = 0, baz = 0, bwx = 0, bwy = 0, bwz = 0;
  Bias() = default;
  Bias(float ax, float ay, float az, float wx, float wy, float wz) : bax(ax), bay(ay), baz(az), bwx(wx), bwy(wy), bwz(wz) {}
};
struct Calib { Mat Tcb{4, 4}; };
struct Preintegrated {
  int owner = -1;
  float dT = 0;
  Mat C{15, 15}, dR{3, 3}, dV{3, 1}, dP{3, 1}, JRg{3, 3}, JVg{3, 3}, JVa{3, 3}, JPg{3, 3}, JPa{3, 3};
  Bias b, bu;
  void SetNewBias(const Bias& bu_) { bu = bu_; log("Preintegrated::SetNewBias " + std::to_string(owner) + " " + std::to_string(bu_.bwx)); }
};

// a mutex that says when it is taken
struct LogMutex {
  void lock() { log("lock"); }
  void unlock() { log("unlock"); }
};

class KeyFrame;
class Map {
 public:
  long n_keyframes = 0;
  LogMutex mMutexMapUpdate;
  long KeyFramesInMap() const { return n_keyframes; }
  void IncreaseChangeIndex() { log("IncreaseChangeIndex"); }
};

class MapPoint {
 public:
  int id = 0;
  float mTrackDepth = 0;
  unsigned long mnBALocalForKF = 0;
  bool bad = false;
  std::map<KeyFrame*, std::tuple<int, int> > obs;
  Mat GetWorldPos() const { return pos; }
  bool isBad() const { return bad; }
  std::map<KeyFrame*, std::tuple<int, int> > GetObservations() const { return obs; }
  void SetWorldPos(const Mat& m, bool, bool) { pos = m; log("SetWorldPos " + std::to_string(id)); }
  void UpdateNormalAndDepth() { log("UpdateNormalAndDepth " + std::to_string(id)); }
  void EraseObservation(KeyFrame* kf);
  void set_pos(float x, float y, float z) { pos = Mat(3, 1); pos.d = {x, y, z}; }
#ifdef MOCK_STRICT_ACCESS
 private:
#endif
  Mat pos{3, 1};
};

class KeyFrame {
 public:
  unsigned long mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
  KeyFrame* mPrevKF = nullptr;
  bool bImu = true, bad = false;
  void* mpCamera2 = nullptr;
  Preintegrated* mpImuPreintegrated = nullptr;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  Calib mImuCalib;
  Map* map = nullptr;
  Map* GetMap() const { return map; }
  bool isBad() const { return bad; }
  std::vector<MapPoint*> GetMapPointMatches() const { return matches; }
  Mat GetImuRotation() const { return R; }
  Mat GetImuPosition() const { return t; }
  Mat GetVelocity() const { return v; }
  Mat GetGyroBias() const { Mat m(3, 1); m.d = {bias.bwx, bias.bwy, bias.bwz}; return m; }
  Mat GetAccBias() const { Mat m(3, 1); m.d = {bias.bax, bias.bay, bias.baz}; return m; }
  Bias GetImuBias() const { return bias; }
  void SetVelocity(const Mat& m) { v = m; log("SetVelocity " + std::to_string(mnId)); }
  void SetNewBias(const Bias& b) { bias = b; log("SetNewBias " + std::to_string(mnId)); }
  void SetPose(const Mat& T, bool) { Tcw = T; log("SetPose " + std::to_string(mnId)); }
  void EraseMapPointMatch(MapPoint* p) { log("EraseMapPointMatch " + std::to_string(mnId) + " " + std::to_string(p->id)); }
#ifdef MOCK_STRICT_ACCESS
 private:
  friend struct Access;
#endif
  std::vector<MapPoint*> matches;
  Mat R{3, 3}, t{3, 1}, v{3, 1}, Tcw{4, 4};
  Bias bias;
};
inline void MapPoint::EraseObservation(KeyFrame* kf) { log("EraseObservation " + std::to_string(kf->mnId) + " " + std::to_string(id)); }

// how the test's driver fills and reads what the glue may not touch directly
struct Access {
  static std::vector<MapPoint*>& matches(KeyFrame& k) { return k.matches; }
  static Mat& R(KeyFrame& k) { return k.R; }
  static Mat& t(KeyFrame& k) { return k.t; }
  static Mat& v(KeyFrame& k) { return k.v; }
  static Mat& Tcw(KeyFrame& k) { return k.Tcw; }
  static Bias& bias(KeyFrame& k) { return k.bias; }
};

}  // namespace mock
