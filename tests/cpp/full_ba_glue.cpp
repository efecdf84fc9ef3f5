// orbgpu::dropin::BundleAdjustment / GlobalBundleAdjustemnt (include/orbgpu_dropin.hpp) over mock keyframes, map points and a map
// that carry exactly the members the reference's Optimizer::BundleAdjustment touches (S/Optimizer.cc:42-447).  The solver is replaced
// by an Ops that records the ba_problem it is handed and returns a known result, so the program needs no device: it checks the
// problem (vertex order, fixed flags, edge order, camera table) and both write-back branches field by field, prints "ok <checks>" and
// exits 0, or names the first check that failed.  Also the stand-alone program of the sanitizer build (tests/test_full_ba_glue.py).
//   full_ba_glue
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "mock_orbslam3.hpp"
#include "orbgpu_dropin.hpp"

using mock::Mat;

struct GMap;
struct GKeyFrame {
  long unsigned mnId = 0, mnUniqueId = 0; uint8_t mnClientId = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<mock::KeyPoint> mvKeysUn; std::vector<float> mvuRight, mvInvLevelSigma2;
  mock::GeometricCamera* mpCamera = nullptr; mock::GeometricCamera* mpCamera2 = nullptr;
  Mat mTcwGBA; long unsigned mnBAGlobalForKF = 0;
  bool bad = false; GMap* map = nullptr; Mat Tcw{4, 4, 4};
  int n_set_pose = 0, n_locked = 0;
  bool isBad() const { return bad; }
  GMap* GetMap() const { return map; }
  Mat GetPose() const { return Tcw; }
  void SetPose(const Mat& T, bool bLock = false) { Tcw = T; n_set_pose++; n_locked += bLock; }
};
struct GMapPoint {
  long unsigned mnId = 0, mnUniqueId = 0;
  Mat mPosGBA; long unsigned mnBAGlobalForKF = 0;
  bool bad = false; Mat pos{3, 1, 4};
  std::map<GKeyFrame*, std::tuple<int, int>> obs;
  int n_set_pos = 0, n_locked = 0, n_normal = 0;
  bool isBad() const { return bad; }
  Mat GetWorldPos() const { return pos; }
  void SetWorldPos(const Mat& X, bool bLock = false) { pos = X; n_set_pos++; n_locked += bLock; }
  void UpdateNormalAndDepth() { n_normal++; }
  std::map<GKeyFrame*, std::tuple<int, int>> GetObservations() const { return obs; }
};
struct GMap {
  uint8_t mnClientId = 1; long unsigned init_id = 0; GKeyFrame* origin = nullptr;
  std::vector<GKeyFrame*> kfs; std::vector<GMapPoint*> mps;
  long unsigned GetInitKFid() const { return init_id; }
  GKeyFrame* GetOriginKF() const { return origin; }
  std::vector<GKeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<GMapPoint*> GetAllMapPoints() const { return mps; }
};

// records the problem, answers with poses whose translation moved by (1 + index) and points that moved by 0.5
struct RecordOps {
  struct Rec {
    ba_problem p{}; std::vector<float> poses, points; std::vector<uint8_t> fixed; std::vector<int32_t> pose_camera;
    std::vector<lba_edge> edges; std::vector<ba_camera> cameras; const volatile bool* stop = nullptr; int calls = 0;
  };
  static Rec& rec() { static Rec r; return r; }
  static int ba(const ba_problem& p, const volatile bool* stop, ba_result& r) {
    Rec& c = rec();
    c.p = p; c.stop = stop; c.calls++;
    c.poses.assign(p.poses, p.poses + 16 * (size_t)p.n_poses); c.points.assign(p.points, p.points + 3 * (size_t)p.n_points);
    c.fixed.assign(p.pose_fixed, p.pose_fixed + p.n_poses); c.pose_camera.assign(p.pose_camera, p.pose_camera + p.n_poses);
    c.edges.assign(p.edges, p.edges + p.n_edges); c.cameras.assign(p.cameras, p.cameras + p.n_cameras);
    for (int i = 0; i < p.n_poses; i++) {
      std::memcpy(r.poses + 16 * (size_t)i, p.poses + 16 * (size_t)i, 64);
      r.poses[16 * (size_t)i + 3] += 1.0f + (float)i;
    }
    for (int j = 0; j < p.n_points; j++) {
      for (int a = 0; a < 3; a++) r.points[3 * (size_t)j + a] = p.points[3 * (size_t)j + a] + 0.5f;
      r.point_included[j] = 0;
    }
    for (int k = 0; k < p.n_edges; k++) r.point_included[p.edges[k].point] = 1;
    r.status = LBA_APPLIED; r.iters = 3;
    return ORBG_OK;
  }
};

static int n_checks = 0;
#define CHECK(cond) do { n_checks++; if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Scene {
  mock::GeometricCamera camA{0, {500.f, 501.f, 320.f, 240.f}}, camB{1, {300.f, 301.f, 256.f, 255.f, 0.01f, 0.02f, 0.03f, 0.04f}};
  GMap map;
  GKeyFrame A, B, C, D, Bad, Outside;
  GMapPoint p0, p1, p2, pBad, pOrphan;
  void keyframe(GKeyFrame& k, long unsigned id, long unsigned uid, uint8_t client, mock::GeometricCamera* cam, float f, float tx) {
    k.mnId = id; k.mnUniqueId = uid; k.mnClientId = client; k.mpCamera = cam; k.map = &map;
    k.fx = f; k.fy = f + 1; k.cx = 320; k.cy = 240; k.mbf = f * 0.1f;
    std::memset(k.Tcw.ptr<float>(0), 0, 64);
    for (int i = 0; i < 4; i++) k.Tcw.ptr<float>(0)[5 * i] = 1.f;
    k.Tcw.ptr<float>(0)[3] = tx;
    k.mvKeysUn = {mock::KeyPoint{{10.f + tx, 20.f}, 31.f, 0.f, 0.f, 0}, mock::KeyPoint{{30.f + tx, 40.f}, 31.f, 0.f, 0.f, 1}};
    k.mvuRight = {5.f + tx, -1.f};                       // feature 0 is a stereo observation, feature 1 a monocular one
    k.mvInvLevelSigma2 = {1.f, 0.6944f};
  }
  void point(GMapPoint& p, long unsigned id, long unsigned uid, float x) {
    p.mnId = id; p.mnUniqueId = uid;
    float* X = p.pos.ptr<float>(0); X[0] = x; X[1] = 2 * x; X[2] = 5.f;
  }
  explicit Scene(bool unique) {
    map.mnClientId = 1; map.init_id = 0; map.origin = &A;
    keyframe(A, 0, 100, 1, &camA, 500.f, 0.f);
    keyframe(B, 1, 101, 1, &camA, 500.f, 0.1f);
    // another agent's keyframes, another camera.  C carries the initial keyframe's mnId in the unique-id run: fixed only if the
    // client matches (:112); ids by mnId must be distinct, so it is keyframe 4 in the other run
    keyframe(C, unique ? 0 : 4, 50, 2, &camB, 300.f, 0.2f);
    keyframe(D, 3, 51, 2, &camB, 300.f, 0.3f);
    keyframe(Bad, 2, 102, 1, &camA, 500.f, 0.4f); Bad.bad = true;
    keyframe(Outside, 9, 999, 1, &camA, 500.f, 0.5f);   // not handed to BundleAdjustment: id > maxKFid
    point(p0, 7, 1007, 0.1f); point(p1, 5, 1005, 0.2f); point(p2, 6, 1006, 0.3f); point(pBad, 1, 1001, 0.4f); point(pOrphan, 8, 1008, 0.5f);
    pBad.bad = true;
    p0.obs[&A] = std::make_tuple(0, -1); p0.obs[&B] = std::make_tuple(1, -1);
    p1.obs[&D] = std::make_tuple(0, -1); p1.obs[&B] = std::make_tuple(0, -1); p1.obs[&C] = std::make_tuple(1, -1);
    p2.obs[&D] = std::make_tuple(1, -1); p2.obs[&Outside] = std::make_tuple(0, -1); p2.obs[&Bad] = std::make_tuple(0, -1);
    pBad.obs[&A] = std::make_tuple(1, -1);
    pOrphan.obs[&Bad] = std::make_tuple(1, -1);
    map.kfs = {&D, &A, &Bad, &C, &B};                   // in no particular order
    map.mps = {&p0, &pOrphan, &pBad, &p2, &p1};
  }
};

static int run(bool unique, bool direct) {
  Scene s(unique);
  bool stop = false;
  const unsigned long nLoopKF = direct ? s.A.mnId : 7;
  RecordOps::rec() = RecordOps::Rec{};
  const int iters = orbgpu::dropin::GlobalBundleAdjustemnt<RecordOps>(&s.map, 10, &stop, unique, nLoopKF, false);
  const RecordOps::Rec& r = RecordOps::rec();
  CHECK(iters == 3 && r.calls == 1 && r.stop == &stop);
  CHECK(r.p.iterations == 10 && r.p.robust == 0);
  // vertices: the four good keyframes in ascending id (unique: C 50, D 51, A 100, B 101; else A 0, B 1, D 3, C 4)
  CHECK(r.p.n_poses == 4);
  GKeyFrame* order_u[4] = {&s.C, &s.D, &s.A, &s.B};
  GKeyFrame* order_n[4] = {&s.A, &s.B, &s.D, &s.C};
  GKeyFrame** kf = unique ? order_u : order_n;
  for (int i = 0; i < 4; i++) {
    CHECK(r.poses[16 * i + 3] == (kf[i] == &s.A ? 0.f : kf[i] == &s.B ? 0.1f : kf[i] == &s.C ? 0.2f : 0.3f));
    CHECK(r.fixed[i] == (kf[i] == &s.A ? 1 : 0));       // C has the initial keyframe's mnId in the unique-id run, but not its client
  }
  // camera table: one entry per distinct camera, in order of first use
  CHECK(r.p.n_cameras == 2);
  const int camOfA = r.pose_camera[unique ? 2 : 0], camOfC = r.pose_camera[unique ? 0 : 3];
  CHECK(camOfA != camOfC && r.pose_camera[unique ? 3 : 1] == camOfA && r.pose_camera[unique ? 1 : 2] == camOfC);
  CHECK(r.cameras[camOfA].fx == 500.f && r.cameras[camOfA].bf == 50.f && r.cameras[camOfA].model.model == 0 && r.cameras[camOfA].model.fy == 501.f);
  CHECK(r.cameras[camOfC].fx == 300.f && r.cameras[camOfC].model.model == 1 && r.cameras[camOfC].model.fx == 300.f && r.cameras[camOfC].model.k[3] == 0.04f);
  // points: the good ones in ascending id -- p1 (5), p2 (6), p0 (7), pOrphan (8); the bad one is left out
  CHECK(r.p.n_points == 4);
  CHECK(r.points[0] == 0.2f && r.points[3] == 0.3f && r.points[6] == 0.1f && r.points[9] == 0.5f);
  // edges: per point, by keyframe vertex id.  p1: B, C, D; p2: D only (Outside is past maxKFid, Bad is bad); p0: A, B; pOrphan: none
  auto col_of = [&](GKeyFrame* k) { for (int i = 0; i < 4; i++) if (kf[i] == k) return i; return -1; };
  struct Want { GKeyFrame* k; int point; int feat; };
  std::vector<Want> want;
  if (unique) want = {{&s.C, 0, 1}, {&s.D, 0, 0}, {&s.B, 0, 0}, {&s.D, 1, 1}, {&s.A, 2, 0}, {&s.B, 2, 1}};
  else want = {{&s.B, 0, 0}, {&s.D, 0, 0}, {&s.C, 0, 1}, {&s.D, 1, 1}, {&s.A, 2, 0}, {&s.B, 2, 1}};
  CHECK(r.p.n_edges == (int)want.size());
  for (size_t k = 0; k < want.size(); k++) {
    const lba_edge& e = r.edges[k];
    const GKeyFrame* w = want[k].k;
    CHECK(e.pose == col_of(want[k].k) && e.point == want[k].point);
    CHECK(e.u == w->mvKeysUn[want[k].feat].pt.x && e.v == w->mvKeysUn[want[k].feat].pt.y && e.ur == w->mvuRight[want[k].feat]);
    CHECK(e.inv_sigma2 == w->mvInvLevelSigma2[want[k].feat]);
  }
  // write-back
  for (int i = 0; i < 4; i++) {
    const float tx_in = r.poses[16 * i + 3], tx_out = tx_in + 1.f + (float)i;
    if (direct) {
      CHECK(kf[i]->n_set_pose == 1 && kf[i]->n_locked == 1 && kf[i]->Tcw.ptr<float>(0)[3] == tx_out && kf[i]->Tcw.ptr<float>(0)[15] == 1.f);
      CHECK(kf[i]->mTcwGBA.empty() && kf[i]->mnBAGlobalForKF == 0);
    } else {
      CHECK(kf[i]->n_set_pose == 0 && kf[i]->Tcw.ptr<float>(0)[3] == tx_in);
      CHECK(kf[i]->mTcwGBA.rows == 4 && kf[i]->mTcwGBA.cols == 4 && kf[i]->mTcwGBA.ptr<float>(0)[3] == tx_out && kf[i]->mnBAGlobalForKF == 7);
    }
  }
  CHECK(s.Bad.n_set_pose == 0 && s.Bad.mTcwGBA.empty() && s.Outside.n_set_pose == 0 && s.Outside.mTcwGBA.empty());
  GMapPoint* pts[3] = {&s.p1, &s.p2, &s.p0};
  const float x_in[3] = {0.2f, 0.3f, 0.1f};
  for (int j = 0; j < 3; j++) {
    if (direct) {
      CHECK(pts[j]->n_set_pos == 1 && pts[j]->n_locked == 1 && pts[j]->n_normal == 1 && pts[j]->pos.ptr<float>(0)[0] == x_in[j] + 0.5f);
      CHECK(pts[j]->mPosGBA.empty());
    } else {
      CHECK(pts[j]->n_set_pos == 0 && pts[j]->n_normal == 0 && pts[j]->pos.ptr<float>(0)[0] == x_in[j]);
      CHECK(pts[j]->mPosGBA.rows == 3 && pts[j]->mPosGBA.ptr<float>(0)[0] == x_in[j] + 0.5f && pts[j]->mPosGBA.ptr<float>(0)[2] == 5.5f);
      CHECK(pts[j]->mnBAGlobalForKF == 7);
    }
  }
  // the point only a bad keyframe observes (nEdges == 0, :289-293) and the bad point: untouched in both branches
  CHECK(s.pOrphan.n_set_pos == 0 && s.pOrphan.mPosGBA.empty() && s.pOrphan.mnBAGlobalForKF == 0 && s.pOrphan.pos.ptr<float>(0)[0] == 0.5f);
  CHECK(s.pBad.n_set_pos == 0 && s.pBad.mPosGBA.empty() && s.pBad.mnBAGlobalForKF == 0);
  return 0;
}

int main() {
  for (int unique = 0; unique < 2; unique++)
    for (int direct = 0; direct < 2; direct++)
      if (run(unique != 0, direct != 0)) { std::printf("in run unique=%d direct=%d\n", unique, direct); return 1; }
  // BundleAdjustment proper, with an empty keyframe list: nothing is read, nothing is solved
  RecordOps::rec() = RecordOps::Rec{};
  std::vector<GKeyFrame*> none; std::vector<GMapPoint*> nonep;
  if (orbgpu::dropin::BundleAdjustment<RecordOps>(none, nonep, 5) != 0 || RecordOps::rec().calls != 0) { std::printf("FAILED empty input\n"); return 1; }
  std::printf("ok %d\n", n_checks);
  return 0;
}
