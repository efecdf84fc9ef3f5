// Stand-ins for what Optimizer::OptimizeEssentialGraph (S/Optimizer.cc:2413-2747) touches: a matrix, a keyframe, a map point, a map and
// a g2o::Sim3, each with exactly the members the glue of include/orbgpu_loopclosing.hpp uses.  Every such member is public in the
// reference and names its line in a `// ref:` note (I/: the reference's include directory, G/: Thirdparty/g2o/g2o); scenes are set up
// through the Test* members.  No Eigen, no OpenCV.
#pragma once
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace mock_eg {

struct Mat {                                           // the slice of cv::Mat the glue uses: a continuous CV_32F matrix
  int rows = 0, cols = 0;
  std::vector<float> data;
  Mat() {}
  Mat(int r, int c) : rows(r), cols(c), data((size_t)r * c, 0.f) {}
};

struct Vector3d { double v[3]; double operator[](int i) const { return v[i]; } };
struct QuatCoeffs { double c[4]; double operator[](int i) const { return c[i]; } };          // x, y, z, w: Eigen's storage order
struct Quaterniond { QuatCoeffs c; const QuatCoeffs& coeffs() const { return c; } };
class Sim3 {
 public:
  Sim3() : r{{{0, 0, 0, 1}}}, t{{0, 0, 0}}, s(1) {}
  Sim3(const double* q, const double* tt, double ss) : r{{{q[0], q[1], q[2], q[3]}}}, t{{tt[0], tt[1], tt[2]}}, s(ss) {}
  const Vector3d& translation() const { return t; }                                          // ref: G/types/sim3.h:280 translation
  const Quaterniond& rotation() const { return r; }                                          // ref: G/types/sim3.h:284 rotation
  const double& scale() const { return s; }                                                  // ref: G/types/sim3.h:288 scale
 protected:
  Quaterniond r; Vector3d t; double s;
};

class KeyFrame {
 public:
  long unsigned int mnId = 0;                                                                // ref: I/KeyFrame.h mnId
  long unsigned int mnUniqueId = 0;                                                          // ref: I/KeyFrame.h mnUniqueId
  bool bImu = false;                                                                         // ref: I/KeyFrame.h bImu
  KeyFrame* mPrevKF = nullptr;                                                               // ref: I/KeyFrame.h mPrevKF
  bool isBad() const { return bad; }                                                         // ref: I/KeyFrame.h isBad
  Mat GetRotation() const { Mat R(3, 3); for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) R.data[3 * a + c] = Tcw.data[4 * a + c]; return R; }   // ref: I/KeyFrame.h GetRotation
  Mat GetTranslation() const { Mat t(3, 1); for (int a = 0; a < 3; a++) t.data[a] = Tcw.data[4 * a + 3]; return t; }                                    // ref: I/KeyFrame.h GetTranslation
  void SetPose(const Mat& T, bool bLock = false) { Tcw = T; n_set_pose++; n_locked += bLock; }                                                         // ref: I/KeyFrame.h SetPose
  KeyFrame* GetParent() const { return parent; }                                             // ref: I/KeyFrame.h GetParent
  bool hasChild(KeyFrame* k) const { return children.count(k) != 0; }                        // ref: I/KeyFrame.h hasChild
  std::set<KeyFrame*> GetLoopEdges() const { return loop_edges; }                            // ref: I/KeyFrame.h GetLoopEdges
  std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w) const {                         // ref: I/KeyFrame.h GetCovisiblesByWeight
    std::vector<KeyFrame*> out;
    for (const auto& c : covis) if (c.second >= w) out.push_back(c.first);
    return out;
  }
  int GetWeight(KeyFrame* k) const { const auto it = weights.find(k); return it == weights.end() ? 0 : it->second; }   // ref: I/KeyFrame.h GetWeight
  // ---- test side
  bool bad = false;
  Mat Tcw{4, 4};
  KeyFrame* parent = nullptr;
  std::set<KeyFrame*> children, loop_edges;
  std::vector<std::pair<KeyFrame*, int>> covis;        // ordered by weight, descending (mvpOrderedConnectedKeyFrames)
  std::map<KeyFrame*, int> weights;
  int n_set_pose = 0, n_locked = 0;
};

class MapPoint {
 public:
  long unsigned int mnCorrectedByKF = 0;                                                     // ref: I/MapPoint.h mnCorrectedByKF
  long unsigned int mnCorrectedReference = 0;                                                // ref: I/MapPoint.h mnCorrectedReference
  bool isBad() const { return bad; }                                                         // ref: I/MapPoint.h isBad
  KeyFrame* GetReferenceKeyFrame() const { return ref; }                                     // ref: I/MapPoint.h GetReferenceKeyFrame
  Mat GetWorldPos() const { return pos; }                                                    // ref: I/MapPoint.h GetWorldPos
  void SetWorldPos(const Mat& X, bool bLock = false) { pos = X; n_set_pos++; n_locked += bLock; }     // ref: I/MapPoint.h SetWorldPos
  void UpdateNormalAndDepth() { n_normal++; }                                                // ref: I/MapPoint.h UpdateNormalAndDepth
  // ---- test side
  bool bad = false;
  KeyFrame* ref = nullptr;
  Mat pos{3, 1};
  int n_set_pos = 0, n_locked = 0, n_normal = 0;
};

struct RecordingMutex {                                // BasicLockable; says whether it is held
  bool held = false; int n_locks = 0;
  void lock() { held = true; n_locks++; }
  void unlock() { held = false; }
};

class Map {
 public:
  RecordingMutex mMutexMapUpdate;                                                            // ref: I/Map.h mMutexMapUpdate (a std::mutex there)
  std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }                             // ref: I/Map.h GetAllKeyFrames
  std::vector<MapPoint*> GetAllMapPoints() const { return mps; }                             // ref: I/Map.h GetAllMapPoints
  long unsigned int GetInitKFid() const { return init_id; }                                  // ref: I/Map.h GetInitKFid
  void IncreaseChangeIndex() { locked_at_change = mMutexMapUpdate.held; change_index++; }   // ref: I/Map.h IncreaseChangeIndex
  // ---- test side
  std::vector<KeyFrame*> kfs;
  std::vector<MapPoint*> mps;
  long unsigned int init_id = 0;
  int change_index = 0;
  bool locked_at_change = false;                       // mMutexMapUpdate was held when the change index moved
};

}  // namespace mock_eg

// the matrix access points include/orbgpu_loopclosing.hpp asks for, declared before it is included
namespace orbgpu { namespace loopclosing {
inline const float* mat_f32(const mock_eg::Mat& m) { return m.data.data(); }
inline void make_mat(mock_eg::Mat& out, int rows, int cols, const float* data) { out = mock_eg::Mat(rows, cols); std::memcpy(out.data.data(), data, sizeof(float) * rows * cols); }
} }
