// The host side of csrc/full_ba.hip under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its own main) that
// tools/full_ba_sanitize.sh links with a sanitized build of full_ba.hip and misc.cpp and runs on the CPU.  It walks what ba_solve does
// before and without a launch -- every refusal, the conversion of the estimate, the solves that run no iteration (iterations == 0, no
// edges, the flag up) -- on problems whose arrays are exactly as long as the problem says, so that a read past an end is seen.
// A problem that needs the device answers ORBG_NO_DEVICE here; on a box with a GPU it is solved (sanitized host code, plain kernels).
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbgpu.h"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

struct Problem {
  std::vector<float> poses, points; std::vector<uint8_t> fixed; std::vector<int32_t> cam; std::vector<lba_edge> edges; std::vector<ba_camera> cameras;
  std::vector<float> oposes, opoints; std::vector<double> chi; std::vector<uint8_t> dep, inc; std::vector<double> trace;
  ba_problem p{}; ba_result r{};
  Problem(int n_poses, int n_points, int obs_per_point) {
    for (int i = 0; i < n_poses; i++) {
      float T[16] = {1, 0, 0, 0.1f * i, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      poses.insert(poses.end(), T, T + 16);
      fixed.push_back(i == 0); cam.push_back(i % 2);
    }
    for (int j = 0; j < n_points; j++) {
      points.insert(points.end(), {0.2f * j - 1.f, 0.1f * j, 4.f + 0.05f * j});
      for (int o = 0; o < obs_per_point && o < n_poses; o++)
        edges.push_back(lba_edge{(j + o) % n_poses, j, 320.f + j, 240.f - j, o % 2 ? -1.f : 300.f + j, 1.f});
    }
    ba_camera a{}; a.fx = 500; a.fy = 500; a.cx = 320; a.cy = 240; a.bf = 40; a.model.model = ORBG_CAM_PINHOLE; a.model.fx = 500; a.model.fy = 500; a.model.cx = 320; a.model.cy = 240;
    ba_camera b = a; b.fx = 300; b.model.model = ORBG_CAM_KANNALA_BRANDT8; b.model.fx = 300;
    cameras = {a, b};
    bind();
  }
  void bind() {
    p.n_poses = (int32_t)fixed.size(); p.n_points = (int32_t)(points.size() / 3); p.n_edges = (int32_t)edges.size(); p.n_cameras = (int32_t)cameras.size();
    p.poses = poses.data(); p.pose_fixed = fixed.data(); p.pose_camera = cam.data(); p.points = points.data(); p.edges = edges.data(); p.cameras = cameras.data();
    p.iterations = 10; p.robust = 1; p.device = 0;
    oposes.assign(poses.size(), -7.f); opoints.assign(points.size(), -7.f); chi.assign(edges.size(), -7.0); dep.assign(edges.size(), 9); inc.assign(points.size() / 3, 9);
    trace.assign(3 * 4, 0.0);
    r = ba_result{};
    r.poses = oposes.data(); r.points = opoints.data(); r.edge_chi2 = chi.data(); r.edge_depth_pos = dep.data(); r.point_included = inc.data();
    r.trace = trace.data(); r.trace_cap = 4;
  }
};

int main() {
  // the solves that run no iteration
  for (int form = 0; form < 3; form++) {
    Problem q(4, 9, 3);
    int32_t flag = INT_MIN;
    uint8_t raised = 1;
    int rc;
    if (form == 0) { q.p.iterations = 0; rc = ba_solve(&q.p, nullptr, &q.r); }
    else if (form == 1) rc = ba_solve(&q.p, &flag, &q.r);
    else rc = ba_solve_b(&q.p, &raised, &q.r);
    EXPECT(rc == ORBG_OK && q.r.iters == 0 && q.r.trace_len == 0);
    EXPECT(q.r.status == (form == 2 ? LBA_ABORTED_BEFORE_OPT : LBA_APPLIED));
    for (size_t i = 0; i < q.points.size(); i++) EXPECT(q.opoints[i] == q.points[i]);
    for (size_t i = 0; i < q.poses.size(); i++) EXPECT(std::fabs(q.oposes[i] - q.poses[i]) < 1e-6f);
    for (size_t k = 0; k < q.edges.size(); k++) EXPECT(q.chi[k] == 0.0 && q.dep[k] == 1);
    for (uint8_t v : q.inc) EXPECT(v == 1);
  }
  { Problem q(3, 0, 0); EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_OK && q.r.iters == 0); }
  { Problem q(0, 0, 0); q.p.n_cameras = 0; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_OK && q.r.iters == 0); }
  // the refusals
  { Problem q(4, 9, 3); q.edges[5].ur = LBA_UR_RIGHT_CAMERA; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }
  { Problem q(4, 9, 3); q.edges[5].pose = 4; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }
  { Problem q(4, 9, 3); q.edges[5].point = -1; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }
  { Problem q(4, 9, 3); q.edges[7].point = 0; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }                   // order rule
  { Problem q(4, 9, 3); q.edges[1].pose = q.edges[0].pose; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }     // twice the same keyframe
  { Problem q(4, 9, 3); q.cam[2] = 2; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }
  { Problem q(4, 9, 3); q.cameras[1].model.model = 5; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }
  { Problem q(4, 9, 3); q.r.poses = nullptr; EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_BAD_ARG); }
  { Problem q(BA_MAX_FREE_POSES + 2, 2, 2); EXPECT(ba_solve(&q.p, nullptr, &q.r) == ORBG_CAP_EXCEEDED); }
  { Problem q(BA_MAX_FREE_POSES + 1, 2, 2); const int rc = ba_solve(&q.p, nullptr, &q.r); EXPECT(rc == ORBG_OK || rc == ORBG_NO_DEVICE); }   // exactly at the cap
  EXPECT(ba_solve(nullptr, nullptr, nullptr) == ORBG_BAD_ARG);
  // a problem that needs the device
  { Problem q(6, 40, 3); const int rc = ba_solve(&q.p, nullptr, &q.r); EXPECT(rc == ORBG_OK || rc == ORBG_NO_DEVICE); std::printf("device solve: %d\n", rc); }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
