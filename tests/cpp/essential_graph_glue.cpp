// orbgpu::loopclosing::OptimizeEssentialGraph (include/orbgpu_loopclosing.hpp) over the mock keyframes, map points and map of
// mock_essential_graph.hpp.  The solver is replaced by an Ops that records the eg_problem it is handed and answers with known
// estimates and points, so the program needs no device.  It reads a scene (tests/test_essential_graph_glue.py writes it from
// tests/essential_graph_model.py's scene dictionary), runs the glue, and prints the recorded problem and everything the write-back
// left, one record per line, for the test to compare field by field with the Python collection.  A second run with an inertial
// keyframe must throw.  Also the stand-alone program of the sanitizer build (tools/essential_graph_sanitize.sh).
//   essential_graph_glue <scene file>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <stdexcept>
#include <vector>

#include "mock_essential_graph.hpp"
#include "orbgpu_loopclosing.hpp"

using namespace mock_eg;

struct RecordOps {
  struct Rec { eg_problem p{}; std::vector<eg_vertex> v; std::vector<eg_edge> e; std::vector<eg_point> x; int calls = 0; };
  static Rec& rec() { static Rec r; return r; }
  // vertex n comes back with t += (n + 1) * (0.5, -0.25, 1) and s * 1.25; a point with a reference moves by 0.5, one without keeps its bits
  static int eg(const eg_problem& p, eg_result& r) {
    Rec& c = rec();
    c.p = p; c.calls++;
    c.v.assign(p.vertices, p.vertices + p.n_vertices); c.e.assign(p.edges, p.edges + p.n_edges); c.x.assign(p.points, p.points + p.n_points);
    for (int n = 0; n < p.n_vertices; n++) {
      double* o = r.estimates + 8 * (size_t)n;
      for (int i = 0; i < 4; i++) o[i] = p.vertices[n].q[i];
      o[4] = p.vertices[n].t[0] + 0.5 * (n + 1); o[5] = p.vertices[n].t[1] - 0.25 * (n + 1); o[6] = p.vertices[n].t[2] + 1.0 * (n + 1);
      o[7] = p.vertices[n].s * 1.25;
    }
    for (int i = 0; i < p.n_points; i++)
      for (int a = 0; a < 3; a++) r.points[3 * (size_t)i + a] = p.points[i].pos[a] + (p.points[i].ref >= 0 ? 0.5f : 0.f);
    r.iters = 7; r.err0 = 3.5; r.errEnd = 0.25;
    return ORBG_OK;
  }
};

static bool rd(FILE* f, long& v) { return std::fscanf(f, "%ld", &v) == 1; }
static bool rd(FILE* f, double& v) { return std::fscanf(f, "%lf", &v) == 1; }
#define RD(x) do { if (!rd(f, x)) { std::printf("FAILED: scene file ended at line %d\n", __LINE__); return 2; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: essential_graph_glue <scene file>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("FAILED: cannot open %s\n", argv[1]); return 2; }
  long n_kf, cur, loop, init_id, fix_scale;
  RD(n_kf); RD(cur); RD(loop); RD(init_id); RD(fix_scale);
  std::vector<KeyFrame> kfs((size_t)n_kf);
  Map map;
  map.init_id = (unsigned long)init_id;
  for (long i = 0; i < n_kf; i++) {
    KeyFrame& k = kfs[i];
    long id, uid, bad, parent, n;
    RD(id); RD(uid); RD(bad); RD(parent);
    k.mnId = (unsigned long)id; k.mnUniqueId = (unsigned long)uid; k.bad = bad != 0; k.parent = parent < 0 ? nullptr : &kfs[parent];
    for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) { double v; RD(v); k.Tcw.data[4 * a + c] = (float)v; }
    for (int a = 0; a < 3; a++) { double v; RD(v); k.Tcw.data[4 * a + 3] = (float)v; }
    k.Tcw.data[15] = 1.f;
    RD(n); for (long j = 0; j < n; j++) { long c; RD(c); k.children.insert(&kfs[c]); }
    RD(n); for (long j = 0; j < n; j++) { long c; RD(c); k.loop_edges.insert(&kfs[c]); }
    RD(n); for (long j = 0; j < n; j++) { long c, w; RD(c); RD(w); k.covis.emplace_back(&kfs[c], (int)w); }
    map.kfs.push_back(&k);
  }
  std::map<KeyFrame*, Sim3> corrected, noncorrected;
  for (auto* m : {&corrected, &noncorrected}) {
    long n; RD(n);
    for (long j = 0; j < n; j++) {
      long i; double q[4], t[3], s;
      RD(i); for (double& v : q) RD(v); for (double& v : t) RD(v); RD(s);
      (*m)[&kfs[i]] = Sim3(q, t, s);
    }
  }
  std::map<KeyFrame*, std::set<KeyFrame*>> loop_connections;
  { long n; RD(n); for (long j = 0; j < n; j++) { long i, m; RD(i); RD(m); for (long k = 0; k < m; k++) { long c; RD(c); loop_connections[&kfs[i]].insert(&kfs[c]); } } }
  { long n; RD(n); for (long j = 0; j < n; j++) { long a, b, w; RD(a); RD(b); RD(w); kfs[a].weights[&kfs[b]] = (int)w; kfs[b].weights[&kfs[a]] = (int)w; } }
  long n_mp; RD(n_mp);
  std::vector<MapPoint> mps((size_t)n_mp);
  for (long j = 0; j < n_mp; j++) {
    long bad, ref, by, cref;
    RD(bad); for (int a = 0; a < 3; a++) { double v; RD(v); mps[j].pos.data[a] = (float)v; } RD(ref); RD(by); RD(cref);
    mps[j].bad = bad != 0; mps[j].ref = &kfs[ref]; mps[j].mnCorrectedByKF = (unsigned long)by; mps[j].mnCorrectedReference = (unsigned long)cref;
    map.mps.push_back(&mps[j]);
  }
  std::fclose(f);

  const bool bFixScale = fix_scale != 0;
  const auto rep = orbgpu::loopclosing::OptimizeEssentialGraph<RecordOps>(&map, &kfs[loop], &kfs[cur], noncorrected, corrected, loop_connections, bFixScale);
  const RecordOps::Rec& c = RecordOps::rec();
  std::printf("problem %d %d %d %d %.17g %u calls %d\n", c.p.n_vertices, c.p.n_edges, c.p.n_points, c.p.iterations, c.p.lambda_init, c.p.struct_size, c.calls);
  for (const eg_vertex& v : c.v)
    std::printf("v %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", v.q[0], v.q[1], v.q[2], v.q[3], v.t[0], v.t[1], v.t[2], v.s, v.fixed, v.fix_scale);
  for (const eg_edge& e : c.e)
    std::printf("e %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", e.vi, e.vj, e.q[0], e.q[1], e.q[2], e.q[3], e.t[0], e.t[1], e.t[2], e.s);
  for (const eg_point& x : c.x) std::printf("p %.9g %.9g %.9g %d\n", x.pos[0], x.pos[1], x.pos[2], x.ref);
  std::printf("report %d %d %d %d %d %d %.17g %.17g\n", rep.n_vertices, rep.n_edges, rep.n_points, rep.dropped_edges, rep.skipped_write_backs, rep.iters,
              rep.err0, rep.errEnd);
  for (long i = 0; i < n_kf; i++) {
    std::printf("kf %ld %d %d %d %d", i, kfs[i].n_set_pose, kfs[i].n_locked, kfs[i].Tcw.rows, kfs[i].Tcw.cols);
    for (float v : kfs[i].Tcw.data) std::printf(" %.9g", v);
    std::printf("\n");
  }
  for (long j = 0; j < n_mp; j++)
    std::printf("mp %ld %d %d %d %.9g %.9g %.9g\n", j, mps[j].n_set_pos, mps[j].n_locked, mps[j].n_normal, mps[j].pos.data[0], mps[j].pos.data[1], mps[j].pos.data[2]);
  std::printf("map %d %d %d %d\n", map.change_index, map.locked_at_change ? 1 : 0, map.mMutexMapUpdate.n_locks, map.mMutexMapUpdate.held ? 1 : 0);

  // D-2: an inertial keyframe with a predecessor is refused before anything is written
  kfs[n_kf - 1].bImu = true; kfs[n_kf - 1].mPrevKF = &kfs[n_kf - 2];
  const int set_before = kfs[0].n_set_pose, calls_before = c.calls;
  bool thrown = false;
  try {
    orbgpu::loopclosing::OptimizeEssentialGraph<RecordOps>(&map, &kfs[loop], &kfs[cur], noncorrected, corrected, loop_connections, bFixScale);
  } catch (const std::logic_error&) { thrown = true; }
  std::printf("inertial %d %d %d\n", thrown ? 1 : 0, kfs[0].n_set_pose - set_before, c.calls - calls_before);
  std::printf("ok\n");
  return 0;
}
