// Mock keyframes, map points and a map with exactly the members the reference's welding BA touches
// (Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag), S/Optimizer.cc:6305-6983), for tests/cpp/weld_ba_glue.cpp.
// Every mutator appends to weld_mock::log(), with the state of the map's mutex at that moment, so that the order of the write-back and
// the lock around it can be read off.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "mock_orbslam3.hpp"

namespace weld_mock {

using mock::Mat;

inline std::vector<std::string>& log() { static std::vector<std::string> l; return l; }

// BasicLockable that knows whether it is held
struct Mutex {
  bool held = false; int n_locks = 0;
  void lock() { held = true; n_locks++; log().push_back("lock"); }
  void unlock() { held = false; log().push_back("unlock"); }
};

struct WMap { Mutex mMutexMapUpdate; };
struct WMapPoint;

struct WKeyFrame {
  std::string name;
  long unsigned mnId = 0, mnUniqueId = 0, mnBALocalForMerge = 0, mnBALocalForKF = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<mock::KeyPoint> mvKeysUn; std::vector<float> mvuRight, mvInvLevelSigma2;
  mock::GeometricCamera* mpCamera = nullptr; mock::GeometricCamera* mpCamera2 = nullptr;
  bool bad = false; WMap* map = nullptr; Mat Tcw{4, 4, 4};
  std::vector<WMapPoint*> matches;                     // mvpMapPoints, by feature index
  int n_set_pose = 0, n_locked = 0;
  bool isBad() const { return bad; }
  WMap* GetMap() const { return map; }
  Mat GetPose() const { return Tcw; }
  std::set<WMapPoint*> GetMapPoints() const { std::set<WMapPoint*> s; for (WMapPoint* p : matches) if (p) s.insert(p); return s; }
  WMapPoint* GetMapPoint(size_t i) const { return i < matches.size() ? matches[i] : nullptr; }
  void EraseMapPointMatch(WMapPoint* p);
  void SetPose(const Mat& T, bool bLock = false) {
    Tcw = T; n_set_pose++; n_locked += bLock;
    log().push_back("SetPose " + name + (map && map->mMutexMapUpdate.held ? " locked" : " UNLOCKED"));
  }
};

struct WMapPoint {
  std::string name;
  long unsigned mnUniqueId = 0, mnBALocalForMerge = 0;
  bool bad = false; WMap* map = nullptr; Mat pos{3, 1, 4};
  std::map<WKeyFrame*, std::tuple<int, int>> obs;
  int n_set_pos = 0, n_locked = 0, n_normal = 0;
  bool isBad() const { return bad; }
  WMap* GetMap() const { return map; }
  Mat GetWorldPos() const { return pos; }
  std::map<WKeyFrame*, std::tuple<int, int>> GetObservations() const { return obs; }
  void EraseObservation(WKeyFrame* kf) {
    obs.erase(kf);
    log().push_back("EraseObservation " + name + " " + kf->name + (map && map->mMutexMapUpdate.held ? " locked" : " UNLOCKED"));
  }
  void SetWorldPos(const Mat& X, bool bLock = false) {
    pos = X; n_set_pos++; n_locked += bLock;
    log().push_back("SetWorldPos " + name + (map && map->mMutexMapUpdate.held ? " locked" : " UNLOCKED"));
  }
  void UpdateNormalAndDepth() { n_normal++; log().push_back("UpdateNormalAndDepth " + name); }
};

inline void WKeyFrame::EraseMapPointMatch(WMapPoint* p) {
  for (WMapPoint*& m : matches) if (m == p) m = nullptr;
  log().push_back("EraseMapPointMatch " + name + " " + p->name + (map && map->mMutexMapUpdate.held ? " locked" : " UNLOCKED"));
}

}  // namespace weld_mock
