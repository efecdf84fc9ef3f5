// orbgpu::dropin::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (include/orbgpu_dropin.hpp), the welding BA of
// LoopClosing::MergeLocal, over the mocks of mock_weld_ba.hpp.  The solver is replaced by an Ops that records the ba_weld_problem it is
// handed and answers with a known result, so the program needs no device: it checks the problem field by field (the run where no
// adjusted keyframe carries the stamp: free poses without edges; the run where one does), the map conditions (a bad keyframe, a keyframe
// of another map, a bad point, a point that turns bad while the solve runs, mnId > maxKFid), both throws, the erase list's order, the
// write-back under the map's mutex and no write-back at all after the early return.  Prints "ok <checks>" and exits 0, or names the
// first check that failed.  Also the stand-alone program of the sanitizer build (tools/weld_ba_sanitize.sh).
//   weld_ba_glue
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mock_weld_ba.hpp"
#include "orbgpu_dropin.hpp"

using namespace weld_mock;

// records the problem; answers with poses whose translation moved by (1 + index), points that moved by 0.5, and chi2 / depth / status
// as the test set them
struct RecordOps {
  struct Rec {
    ba_weld_problem p{}; std::vector<float> poses, points; std::vector<uint8_t> fixed; std::vector<int32_t> pose_camera;
    std::vector<lba_edge> edges; std::vector<ba_camera> cameras; const volatile bool* stop = nullptr; int calls = 0;
    std::vector<double> chi2; std::vector<uint8_t> depth_neg; int status = LBA_APPLIED; WMapPoint* turns_bad = nullptr;
    bool had_outputs = false;
  };
  static Rec& rec() { static Rec r; return r; }
  static int ba_weld(const ba_weld_problem& w, const volatile bool* stop, ba_weld_result& r) {
    Rec& c = rec();
    const ba_problem& p = w.ba;
    c.p = w; c.stop = stop; c.calls++;
    c.poses.assign(p.poses, p.poses + 16 * (size_t)p.n_poses); c.points.assign(p.points, p.points + 3 * (size_t)p.n_points);
    c.fixed.assign(p.pose_fixed, p.pose_fixed + p.n_poses); c.pose_camera.assign(p.pose_camera, p.pose_camera + p.n_poses);
    c.edges.assign(p.edges, p.edges + p.n_edges); c.cameras.assign(p.cameras, p.cameras + p.n_cameras);
    c.had_outputs = r.struct_size == sizeof(ba_weld_result) && r.ba.poses && r.ba.points && r.ba.edge_chi2 && r.ba.edge_depth_pos && r.edge_level;
    for (int i = 0; i < p.n_poses; i++) {
      std::memcpy(r.ba.poses + 16 * (size_t)i, p.poses + 16 * (size_t)i, 64);
      r.ba.poses[16 * (size_t)i + 3] += 1.0f + (float)i;
    }
    for (int j = 0; j < p.n_points; j++)
      for (int a = 0; a < 3; a++) r.ba.points[3 * (size_t)j + a] = p.points[3 * (size_t)j + a] + 0.5f;
    for (int k = 0; k < p.n_edges; k++) {
      r.ba.edge_chi2[k] = (size_t)k < c.chi2.size() ? c.chi2[k] : 0.0;
      r.ba.edge_depth_pos[k] = (size_t)k < c.depth_neg.size() && c.depth_neg[k] ? 0 : 1;
      r.edge_level[k] = 0;
    }
    r.ba.status = c.status; r.ba.iters = 5; r.iters_second = 10; r.rounds_run = c.status == LBA_APPLIED ? 2 : 0;
    if (c.turns_bad) c.turns_bad->bad = true;            // while the solve runs, another thread culls a point
    return ORBG_OK;
  }
};

static int n_checks = 0;
#define CHECK(cond) do { n_checks++; if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Scene {
  mock::GeometricCamera camA{0, {500.f, 501.f, 320.f, 240.f}}, camB{1, {300.f, 301.f, 256.f, 255.f, 0.01f, 0.02f, 0.03f, 0.04f}};
  WMap map, other;
  // fixed: F0 (the main keyframe), F1, FBad (bad), FOther (another map); adjusted: A0, A1, ABad (bad)
  // Late: mnId past maxKFid, carries the stamp; Stray: carries the stamp, is in neither list (used by the throw run only)
  WKeyFrame F0, F1, FBad, FOther, A0, A1, ABad, Late, Stray;
  // (members in this order: GetMapPoints() walks a std::set by address, so the points are collected p0, p1, pTurn, ...)
  WMapPoint p0, p1, pTurn, pBad, pOther, pFree;
  void keyframe(WKeyFrame& k, const char* name, long unsigned id, long unsigned uid, WMap* m, mock::GeometricCamera* cam, float f, float tx) {
    k.name = name; k.mnId = id; k.mnUniqueId = uid; k.map = m; k.mpCamera = cam;
    k.fx = f; k.fy = f + 1; k.cx = 320; k.cy = 240; k.mbf = f * 0.1f;
    std::memset(k.Tcw.ptr<float>(0), 0, 64);
    for (int i = 0; i < 4; i++) k.Tcw.ptr<float>(0)[5 * i] = 1.f;
    k.Tcw.ptr<float>(0)[3] = tx;
    k.mvInvLevelSigma2 = {1.f, 0.6944f};
  }
  void point(WMapPoint& p, const char* name, long unsigned uid, WMap* m, float x) {
    p.name = name; p.mnUniqueId = uid; p.map = m;
    float* X = p.pos.ptr<float>(0); X[0] = x; X[1] = 2 * x; X[2] = 5.f;
  }
  void see(WKeyFrame& k, WMapPoint& p, bool stereo) {
    const int i = (int)k.mvKeysUn.size();
    const float u = 10.f * (float)i + (float)k.mnUniqueId;
    k.mvKeysUn.push_back(mock::KeyPoint{{u, 20.f + (float)i}, 31.f, 0.f, 0.f, i % 2});
    k.mvuRight.push_back(stereo ? u - 3.f : -1.f);
    k.matches.push_back(&p);
    p.obs[&k] = std::make_tuple(i, -1);
  }
  Scene() {
    keyframe(F0, "F0", 10, 100, &map, &camA, 500.f, 0.f);
    keyframe(F1, "F1", 11, 101, &map, &camA, 500.f, 0.1f);
    keyframe(FBad, "FBad", 12, 102, &map, &camA, 500.f, 0.2f); FBad.bad = true;
    keyframe(FOther, "FOther", 13, 103, &other, &camA, 500.f, 0.3f);
    keyframe(A0, "A0", 5, 50, &map, &camB, 300.f, 0.4f);        // another agent's keyframes: another camera, smaller unique ids
    keyframe(A1, "A1", 6, 51, &map, &camB, 300.f, 0.5f);
    keyframe(ABad, "ABad", 7, 52, &map, &camB, 300.f, 0.6f); ABad.bad = true;
    keyframe(Late, "Late", 99, 60, &map, &camA, 500.f, 0.7f); Late.mnBALocalForMerge = 100;
    keyframe(Stray, "Stray", 8, 61, &map, &camA, 500.f, 0.8f);
    point(p0, "p0", 1000, &map, 0.1f); point(p1, "p1", 999, &map, 0.2f); point(pTurn, "pTurn", 998, &map, 0.3f);
    point(pBad, "pBad", 997, &map, 0.4f); pBad.bad = true;
    point(pOther, "pOther", 996, &other, 0.5f);
    point(pFree, "pFree", 995, &map, 0.6f);                     // seen by adjusted keyframes only
    see(F0, p0, true); see(F0, p1, false); see(F0, pTurn, false); see(F0, pBad, false); see(F0, pOther, false);
    see(F1, p0, false); see(F1, p1, true); see(F1, pTurn, true);
    see(A0, p0, true); see(A0, pFree, false);
    see(A1, p1, false); see(A1, pFree, true);
    see(FBad, p0, false); see(ABad, p1, false); see(FOther, p1, false);
    see(Late, p1, true);
  }
};

static bool in_log(const std::string& s) { for (const auto& l : log()) if (l == s) return true; return false; }
static int index_in_log(const std::string& s) { for (size_t i = 0; i < log().size(); i++) if (log()[i] == s) return (int)i; return -1; }

// stamped: A0 carries mnBALocalForMerge == pMainKF->mnUniqueId before the call
static int run(bool stamped) {
  Scene s;
  log().clear();
  if (stamped) s.A0.mnBALocalForMerge = 100;
  bool stop = false;
  RecordOps::rec() = RecordOps::Rec{};
  RecordOps::Rec& r = RecordOps::rec();
  r.turns_bad = &s.pTurn;
  // every edge fails the final check: chi2 above the threshold, except the last one, which fails by its depth alone
  r.chi2.assign(16, 100.0);
  const int n_edges = stamped ? 8 : 6;
  r.chi2[n_edges - 1] = 0.0; r.depth_neg.assign(16, 0); r.depth_neg[n_edges - 1] = 1;
  const int status = orbgpu::dropin::LocalBundleAdjustment<RecordOps>(&s.F0, {&s.A0, &s.ABad, &s.A1}, {&s.F1, &s.FBad, &s.FOther, &s.F0}, &stop);
  CHECK(status == LBA_APPLIED && r.calls == 1 && r.stop == &stop && r.had_outputs);
  const ba_problem& p = r.p.ba;
  CHECK(r.p.struct_size == sizeof(ba_weld_problem) && p.iterations == 5 && r.p.iterations_second == 10);
  CHECK(r.p.chi2_mono == 5.991 && r.p.chi2_stereo == 7.815 && p.device == 0);
  // stamps: mnBALocalForMerge on the fixed keyframes that are good and of this map, mnBALocalForKF on the adjusted ones
  CHECK(s.F0.mnBALocalForMerge == 100 && s.F1.mnBALocalForMerge == 100 && s.FBad.mnBALocalForMerge == 0 && s.FOther.mnBALocalForMerge == 0);
  CHECK(s.A0.mnBALocalForKF == 100 && s.A1.mnBALocalForKF == 100 && s.ABad.mnBALocalForKF == 0 && s.F0.mnBALocalForKF == 0);
  CHECK(s.A0.mnBALocalForMerge == (stamped ? 100u : 0u) && s.A1.mnBALocalForMerge == 0);
  CHECK(s.p0.mnBALocalForMerge == 100 && s.p1.mnBALocalForMerge == 100 && s.pTurn.mnBALocalForMerge == 100 && s.pFree.mnBALocalForMerge == 100);
  CHECK(s.pBad.mnBALocalForMerge == 0 && s.pOther.mnBALocalForMerge == 0);
  // vertices: the four good keyframes of this map by mnUniqueId -- A0 50, A1 51, F0 100, F1 101 -- the adjusted ones free
  CHECK(p.n_poses == 4);
  const float tx[4] = {0.4f, 0.5f, 0.f, 0.1f};
  for (int i = 0; i < 4; i++) { CHECK(r.poses[16 * i + 3] == tx[i] && r.poses[16 * i + 15] == 1.f); CHECK(r.fixed[i] == (i >= 2 ? 1 : 0)); }
  CHECK(p.n_cameras == 2 && r.pose_camera[0] == r.pose_camera[1] && r.pose_camera[2] == r.pose_camera[3] && r.pose_camera[0] != r.pose_camera[2]);
  CHECK(r.cameras[r.pose_camera[0]].fx == 300.f && r.cameras[r.pose_camera[0]].bf == 30.f && r.cameras[r.pose_camera[0]].model.model == 1);
  CHECK(r.cameras[r.pose_camera[2]].fx == 500.f && r.cameras[r.pose_camera[2]].model.model == 0 && r.cameras[r.pose_camera[2]].model.fy == 501.f);
  // points: pFree 995, pTurn 998, p1 999, p0 1000 (the bad one and the other map's are left out)
  CHECK(p.n_points == 4);
  CHECK(r.points[0] == 0.6f && r.points[3] == 0.3f && r.points[6] == 0.2f && r.points[9] == 0.1f && r.points[2] == 5.f);
  // edges: per point, by keyframe vertex id, from the keyframes that carry the stamp.  Not stamped: no edge of A0 or A1 -- pFree has
  // none at all, the free poses have none.  Late (mnId 99 > maxKFid 11) carries the stamp and is skipped; FBad, ABad, FOther too
  struct Want { WKeyFrame* k; int pose; int point; int feat; };
  std::vector<Want> want;
  if (stamped) want = {{&s.A0, 0, 0, 1}, {&s.F0, 2, 1, 2}, {&s.F1, 3, 1, 2}, {&s.F0, 2, 2, 1}, {&s.F1, 3, 2, 1}, {&s.A0, 0, 3, 0}, {&s.F0, 2, 3, 0}, {&s.F1, 3, 3, 0}};
  else want = {{&s.F0, 2, 1, 2}, {&s.F1, 3, 1, 2}, {&s.F0, 2, 2, 1}, {&s.F1, 3, 2, 1}, {&s.F0, 2, 3, 0}, {&s.F1, 3, 3, 0}};
  CHECK(p.n_edges == (int)want.size());
  for (size_t k = 0; k < want.size(); k++) {
    const lba_edge& e = r.edges[k];
    const WKeyFrame* w = want[k].k;
    CHECK(e.pose == want[k].pose && e.point == want[k].point);
    CHECK(e.u == w->mvKeysUn[want[k].feat].pt.x && e.v == w->mvKeysUn[want[k].feat].pt.y && e.ur == w->mvuRight[want[k].feat]);
    CHECK(e.inv_sigma2 == w->mvInvLevelSigma2[want[k].feat % 2]);
  }
  if (!stamped) for (const lba_edge& e : r.edges) CHECK(r.fixed[e.pose] == 1);
  // the erase list: monocular edges first, then stereo, each in CREATION order (points as collected: p0, p1, pTurn, ..., pFree), and
  // pTurn -- bad by the time of the final check -- not at all.  Every erase happens under the mutex, before any SetPose
  std::vector<std::string> erases;
  for (const auto& l : log()) if (l.rfind("EraseMapPointMatch", 0) == 0) erases.push_back(l);
  std::vector<std::string> want_erases;
  if (stamped) want_erases = {"EraseMapPointMatch F1 p0 locked", "EraseMapPointMatch F0 p1 locked", "EraseMapPointMatch A0 pFree locked",
                              "EraseMapPointMatch A0 p0 locked", "EraseMapPointMatch F0 p0 locked", "EraseMapPointMatch F1 p1 locked"};
  else want_erases = {"EraseMapPointMatch F1 p0 locked", "EraseMapPointMatch F0 p1 locked", "EraseMapPointMatch F0 p0 locked", "EraseMapPointMatch F1 p1 locked"};
  CHECK(erases == want_erases);
  for (size_t i = 0; i + 1 < log().size(); i++)
    if (log()[i].rfind("EraseMapPointMatch", 0) == 0) CHECK(log()[i + 1].rfind("EraseObservation", 0) == 0 && log()[i + 1].find(" locked") != std::string::npos);
  CHECK(s.F1.GetMapPoint(0) == nullptr && s.p0.obs.count(&s.F1) == 0 && s.F0.GetMapPoint(2) == &s.pTurn && s.pTurn.obs.count(&s.F0) == 1);
  // write-back: one lock, taken before the first mutation and released after the last; the adjusted keyframes that are not bad get
  // their pose (locked pose), the collected points that are not bad their position, pFree -- a vertex without an edge -- included
  CHECK(s.map.mMutexMapUpdate.n_locks == 1 && !s.map.mMutexMapUpdate.held && log().front() == "lock" && log().back() == "unlock");
  for (const auto& l : log()) CHECK(l.find("UNLOCKED") == std::string::npos);
  CHECK(index_in_log("SetPose A0 locked") > index_in_log(want_erases.back()) && index_in_log("SetPose A1 locked") > index_in_log("SetPose A0 locked"));
  CHECK(index_in_log("SetWorldPos p0 locked") > index_in_log("SetPose A1 locked"));
  CHECK(s.A0.n_set_pose == 1 && s.A0.n_locked == 1 && s.A0.Tcw.ptr<float>(0)[3] == 0.4f + 1.f && s.A0.Tcw.ptr<float>(0)[15] == 1.f);
  CHECK(s.A1.n_set_pose == 1 && s.A1.Tcw.ptr<float>(0)[3] == 0.5f + 2.f);
  CHECK(s.F0.n_set_pose == 0 && s.F1.n_set_pose == 0 && s.ABad.n_set_pose == 0 && s.FBad.n_set_pose == 0 && s.FOther.n_set_pose == 0 && s.Late.n_set_pose == 0);
  WMapPoint* good[3] = {&s.p0, &s.p1, &s.pFree};
  const float x_in[3] = {0.1f, 0.2f, 0.6f};
  for (int j = 0; j < 3; j++)
    CHECK(good[j]->n_set_pos == 1 && good[j]->n_locked == 1 && good[j]->n_normal == 1 && good[j]->pos.ptr<float>(0)[0] == x_in[j] + 0.5f &&
          good[j]->pos.ptr<float>(0)[2] == 5.5f);
  CHECK(s.pTurn.n_set_pos == 0 && s.pBad.n_set_pos == 0 && s.pOther.n_set_pos == 0 && s.pTurn.pos.ptr<float>(0)[0] == 0.3f);
  CHECK(in_log("UpdateNormalAndDepth pFree") && !in_log("UpdateNormalAndDepth pTurn"));
  return 0;
}

static int run_early_return() {
  Scene s;
  log().clear();
  bool stop = true;
  RecordOps::rec() = RecordOps::Rec{};
  RecordOps::rec().status = LBA_ABORTED_BEFORE_OPT;
  RecordOps::rec().chi2.assign(16, 100.0);
  const int status = orbgpu::dropin::LocalBundleAdjustment<RecordOps>(&s.F0, {&s.A0, &s.A1}, {&s.F0, &s.F1}, &stop);
  CHECK(status == LBA_ABORTED_BEFORE_OPT && RecordOps::rec().calls == 1 && RecordOps::rec().stop == &stop);
  CHECK(log().empty() && s.map.mMutexMapUpdate.n_locks == 0);              // no erase, no pose, no point, no lock
  CHECK(s.A0.n_set_pose == 0 && s.p0.n_set_pos == 0 && s.F1.GetMapPoint(0) == &s.p0);
  CHECK(s.F0.mnBALocalForMerge == 100 && s.A0.mnBALocalForKF == 100);      // (the stamps of the collection stay, as in the reference)
  return 0;
}

static int run_throws() {
  {
    Scene s;                                             // Stray carries the stamp, is within maxKFid, is in neither list, observes p0
    s.Stray.mnBALocalForMerge = 100;
    s.see(s.Stray, s.p0, false);
    bool threw = false;
    RecordOps::rec() = RecordOps::Rec{};
    try { orbgpu::dropin::LocalBundleAdjustment<RecordOps>(&s.F0, {&s.A0, &s.A1}, {&s.F0, &s.F1}, nullptr); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("no vertex") != std::string::npos; }
    CHECK(threw && RecordOps::rec().calls == 0);
  }
  {
    Scene s;                                             // a point with a keyframe's mnUniqueId
    s.p1.mnUniqueId = 101;
    bool threw = false;
    RecordOps::rec() = RecordOps::Rec{};
    try { orbgpu::dropin::LocalBundleAdjustment<RecordOps>(&s.F0, {&s.A0, &s.A1}, {&s.F0, &s.F1}, nullptr); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("mnUniqueId of another vertex") != std::string::npos; }
    CHECK(threw && RecordOps::rec().calls == 0);
  }
  {
    Scene s;                                             // an observation by the second camera of a two-camera keyframe
    s.F1.mpCamera2 = &s.camB;
    s.p0.obs[&s.F1] = std::make_tuple(0, 3);
    bool threw = false;
    RecordOps::rec() = RecordOps::Rec{};
    try { orbgpu::dropin::LocalBundleAdjustment<RecordOps>(&s.F0, {&s.A0, &s.A1}, {&s.F0, &s.F1}, nullptr); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("mpCamera2") != std::string::npos; }
    CHECK(threw && RecordOps::rec().calls == 0);
  }
  return 0;
}

int main() {
  for (int stamped = 0; stamped < 2; stamped++)
    if (run(stamped != 0)) { std::printf("in run stamped=%d\n", stamped); return 1; }
  if (run_early_return()) { std::printf("in run_early_return\n"); return 1; }
  if (run_throws()) { std::printf("in run_throws\n"); return 1; }
  std::printf("ok %d\n", n_checks);
  return 0;
}
