// orbgpu::LocalInertialBA (orbgpu_inertial.hpp) over the mock types of mock_inertial_ba.hpp.  Builds a small map from its arguments,
// calls the glue with the library call replaced by one that records the problem and returns a canned result, and dumps what the
// glue handed over, the event log (the order of every visible effect) and the stamps it left.  tests/test_inertial_ba_glue.py reads it.
//   inertial_ba_glue <chain> <keyframes in map> <extra observers> <failed> <large> <rec_init> <no-imu keyframe id or -1> [<oddities>]
// oddities, a sum of: 1 point 5 is bad; 2 the first extra observer is bad; 4 the second extra observer belongs to another map;
// 8 pKF's first observation of its first point has no left index; 16 the first extra observer has a second camera
// chain keyframes have ids 1 .. chain, each the mPrevKF of the next; pKF is the last.  Point p (0 .. 11) is seen by chain keyframes
// p % chain and (p + 1) % chain (+1: ids), point 3 stereo; every extra observer (ids 1001 ..) sees one point of its own together with
// pKF, and point 0 as well.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "mock_inertial_ba.hpp"
#include "orbgpu_inertial.hpp"

using namespace mock;

static int g_failed = 0;

struct RecordOps {
  static int information(const float* C, double* i9, double* ig, double* ia) {
    for (int i = 0; i < 81; i++) i9[i] = C[0] + i;
    for (int i = 0; i < 9; i++) { ig[i] = C[0] + 100 + i; ia[i] = C[0] + 200 + i; }
    return ORBG_OK;
  }
  static int solve(const inertial_ba_problem& p, inertial_ba_result& r) {
    printf("head %u %d %d %d %d %d %d\n", p.struct_size == sizeof(p), p.n_keyframes, p.n_points, p.n_edges, p.rec_init, p.large, p.device);
    printf("cam %.9g %.9g %.9g %.9g %.9g\nTcb", p.fx, p.fy, p.cx, p.cy, p.bf);
    for (int i = 0; i < 12; i++) printf(" %.9g", p.Tcb[i]);
    printf("\n");
    for (int i = 0; i < p.n_keyframes; i++) {
      const inertial_ba_keyframe& k = p.keyframes[i];
      printf("kf %d fixed %d imu %d link %d prev %d last %d twb0 %.9g vwb0 %.9g bg0 %.9g ba0 %.9g dT %.9g info %.17g %.17g %.17g\n", i, k.fixed, k.imu, k.link,
             k.prev, k.last_in_window, k.state.twb[0], k.state.vwb[0], k.state.bg[0], k.state.ba[0], k.preint.dT, k.info9[0], k.infoG[0], k.infoA[0]);
    }
    for (int l = 0; l < p.n_points; l++) printf("pt %d %.9g %d\n", l, p.points[3 * l], p.close[l]);
    for (int k = 0; k < p.n_edges; k++)
      printf("edge %d kf %d pt %d u %.9g v %.9g ur %.9g w %.9g\n", k, p.edges[k].pose, p.edges[k].point, p.edges[k].u, p.edges[k].v, p.edges[k].ur,
             p.edges[k].inv_sigma2);
    // a canned result: keyframe i at twb = (10 + i, 0, 0) with the identity as Rwb, points moved by +1, every third edge an outlier
    for (int i = 0; i < p.n_keyframes; i++) {
      inertial_ba_state& s = r.states[i];
      memset(&s, 0, sizeof(s));
      s.Rwb[0] = s.Rwb[4] = s.Rwb[8] = 1;
      s.twb[0] = 10 + i; s.vwb[0] = 20 + i; s.bg[0] = 0.5 + i; s.ba[0] = -0.5 - i;
    }
    for (int l = 0; l < 3 * p.n_points; l++) r.points[l] = p.points[l] + 1;
    for (int k = 0; k < p.n_edges; k++) r.edge_outlier[k] = k % 3 == 0;
    r.failed = g_failed;
    log("solve");
    return ORBG_OK;
  }
};

int main(int argc, char** argv) {
  if (argc < 8) { fprintf(stderr, "usage: %s chain in_map extras failed large rec_init no_imu_id\n", argv[0]); return 2; }
  const int chain = atoi(argv[1]), in_map = atoi(argv[2]), extras = atoi(argv[3]);
  g_failed = atoi(argv[4]);
  const bool large = atoi(argv[5]) != 0, rec_init = atoi(argv[6]) != 0;
  const int no_imu = atoi(argv[7]);
  const int odd = argc > 8 ? atoi(argv[8]) : 0;
  Map map, other_map;
  map.n_keyframes = in_map;
  const int n_pts = 12 + extras;
  std::vector<KeyFrame> kfs((size_t)chain + extras);            // one array: the observation maps iterate in index order
  std::vector<MapPoint> pts((size_t)n_pts);
  std::vector<std::unique_ptr<Preintegrated> > pre;
  for (int l = 0; l < n_pts; l++) { pts[l].id = l; pts[l].set_pos(100.f + l, 0.f, 5.f); pts[l].mTrackDepth = l % 2 ? 5.f : 20.f; }
  for (size_t i = 0; i < kfs.size(); i++) {
    KeyFrame& k = kfs[i];
    const bool in_chain = (int)i < chain;
    k.mnId = in_chain ? i + 1 : 1001 + (i - chain);
    k.map = &map;
    k.bImu = in_chain && (int)k.mnId != no_imu;
    k.fx = 458.f; k.fy = 457.f; k.cx = 367.f; k.cy = 248.f; k.mbf = 47.9f;
    for (int a = 0; a < 4; a++) k.mImuCalib.Tcb.d[5 * a] = 1.f;
    k.mImuCalib.Tcb.d[3] = 0.25f;                                // tcb = (0.25, 0, 0)
    k.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
    Access::R(k).d = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Access::t(k).d = {(float)k.mnId, 0, 0};
    Access::v(k).d = {(float)k.mnId + 0.5f, 0, 0};
    Access::bias(k) = Bias(-(float)k.mnId, 0, 0, (float)k.mnId + 0.25f, 0, 0);
    if (in_chain && i > 0) {
      k.mPrevKF = &kfs[i - 1];
      pre.emplace_back(new Preintegrated());
      pre.back()->owner = (int)k.mnId; pre.back()->dT = 0.01f * k.mnId; pre.back()->C.d[0] = (float)k.mnId;
      k.mpImuPreintegrated = pre.back().get();
    }
  }
  auto observe = [&](KeyFrame& k, MapPoint& p, bool stereo) {
    const int f = (int)k.mvKeysUn.size();
    KeyPoint kp; kp.pt.x = 10.f * k.mnId + p.id; kp.pt.y = 1000.f + p.id; kp.octave = p.id % 3;
    k.mvKeysUn.push_back(kp);
    k.mvuRight.push_back(stereo ? kp.pt.x - 3.f : -1.f);
    Access::matches(k).push_back(&p);
    p.obs[&k] = std::make_tuple(f, -1);
  };
  for (int l = 0; l < 12; l++) {
    observe(kfs[l % chain], pts[l], l == 3);
    if (chain > 1) observe(kfs[(l + 1) % chain], pts[l], l == 3);
  }
  KeyFrame* pKF = &kfs[chain - 1];
  for (int x = 0; x < extras; x++) {
    observe(*pKF, pts[12 + x], false);
    observe(kfs[chain + x], pts[12 + x], false);
    observe(kfs[chain + x], pts[0], false);
  }
  static int second_camera;
  if (odd & 1) pts[5].bad = true;
  if ((odd & 2) && extras > 0) kfs[chain].bad = true;
  if ((odd & 4) && extras > 1) kfs[chain + 1].map = &other_map;
  if ((odd & 8) && extras > 0) std::get<0>(pts[12].obs[pKF]) = -1;
  if ((odd & 16) && extras > 0) kfs[chain].mpCamera2 = &second_camera;
  bool stop = false;
  try {
    orbgpu::LocalInertialBA<RecordOps>(pKF, &stop, &map, large, rec_init);
  } catch (const std::exception& e) {
    printf("threw %s\n", e.what());
  }
  for (const std::string& e : events()) printf("event %s\n", e.c_str());
  for (KeyFrame& k : kfs) {
    const Bias b = k.GetImuBias();
    printf("stamp_kf %lu %lu %lu v %.9g bias %.9g %.9g T %.9g %.9g\n", k.mnId, k.mnBALocalForKF, k.mnBAFixedForKF, k.GetVelocity().d[0], b.bwx, b.bax,
           Access::Tcw(k).d[0], Access::Tcw(k).d[3]);
  }
  for (MapPoint& p : pts) printf("stamp_pt %d %lu pos %.9g\n", p.id, p.mnBALocalForKF, p.GetWorldPos().d[0]);
  return 0;
}
