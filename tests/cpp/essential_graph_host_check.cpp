// What eg_solve (include/orbgpu.h) does before and without a launch, as a stand-alone program for the sanitizer build of
// tools/essential_graph_sanitize.sh: the refusals, the cap, and the problems that are answered on the host (no free vertex, no edge, no
// iteration).  Needs no device and uses none.  Prints "ok <checks>" and exits 0, or names the first check that failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbgpu.h"

static int n_checks = 0;
#define CHECK(cond) do { n_checks++; if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  const int V = 5;
  std::vector<eg_vertex> v(V);
  std::vector<eg_edge> e;
  for (int i = 0; i < V; i++) {
    v[i] = eg_vertex{{0, 0, 0, 1}, {-1.0 * i, 0.01 * i, 0}, 1.0, i == 0, 0};
    if (i > 0) e.push_back(eg_edge{i, i - 1, {0, 0, 0, 1}, {1.0, 0, 0}, 1.0});
  }
  e.push_back(eg_edge{V - 1, 0, {0, 0.01, 0, 0.99995}, {V - 1.0, 0, 0}, 1.02});
  std::vector<eg_point> x = {eg_point{{1.f, 2.f, 3.f}, 2}, eg_point{{-1.f, 0.5f, 4.f}, -1}};
  std::vector<double> est(8 * V), err(7 * e.size()), trace(4 * 20);
  std::vector<float> pts(3 * x.size());
  eg_problem p{};
  p.struct_size = sizeof(p); p.n_vertices = V; p.vertices = v.data(); p.n_edges = (int)e.size(); p.edges = e.data(); p.iterations = 20;
  p.lambda_init = 1e-16; p.n_points = (int)x.size(); p.points = x.data(); p.device = 0;
  eg_result r{};
  r.struct_size = sizeof(r); r.estimates = est.data(); r.points = pts.data(); r.trace = trace.data(); r.trace_cap = 20; r.edge_error0 = err.data();

  // refusals, before a device is looked for
  { eg_problem q = p; q.struct_size -= 1; CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { eg_result s = r; s.struct_size = 4; CHECK(eg_solve(&p, &s) == ORBG_BAD_ARG); }
  CHECK(eg_solve(nullptr, &r) == ORBG_BAD_ARG && eg_solve(&p, nullptr) == ORBG_BAD_ARG);
  { auto e2 = e; e2[1].vj = V; eg_problem q = p; q.edges = e2.data(); CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { auto e2 = e; e2[1].vi = -1; eg_problem q = p; q.edges = e2.data(); CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { auto e2 = e; e2[2].s = 0; eg_problem q = p; q.edges = e2.data(); CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { auto v2 = v; v2[3].t[1] = NAN; eg_problem q = p; q.vertices = v2.data(); CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { auto v2 = v; v2[3].s = -2; eg_problem q = p; q.vertices = v2.data(); CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { auto x2 = x; x2[0].ref = V; eg_problem q = p; q.points = x2.data(); CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  { eg_problem q = p; q.n_vertices = -1; CHECK(eg_solve(&q, &r) == ORBG_BAD_ARG); }
  {
    const int n = EG_MAX_FREE_KEYFRAMES + 2;
    std::vector<eg_vertex> big(n, v[1]);
    big[0].fixed = 1;
    std::vector<double> est2(8 * (size_t)n);
    eg_problem q = p; q.n_vertices = n; q.vertices = big.data(); q.n_points = 0;
    eg_result s = r; s.estimates = est2.data(); s.edge_error0 = nullptr;
    CHECK(eg_solve(&q, &s) == ORBG_CAP_EXCEEDED);
    big[1].fixed = 1; q.iterations = 0;
    CHECK(eg_solve(&q, &s) == ORBG_OK && s.iters == 0);
  }
  // answered on the host
  for (int variant = 0; variant < 3; variant++) {
    eg_problem q = p;
    auto v2 = v;
    if (variant == 0) q.iterations = 0;
    if (variant == 1) { for (auto& a : v2) a.fixed = 1; q.vertices = v2.data(); }
    if (variant == 2) q.n_edges = 0;
    std::fill(est.begin(), est.end(), -7.0);
    CHECK(eg_solve(&q, &r) == ORBG_OK);
    CHECK(r.iters == 0 && r.trace_len == 0 && r.err0 == r.errEnd);
    CHECK(variant == 2 ? r.err0 == 0 : r.err0 > 1e-4);
    for (int i = 0; i < V; i++) CHECK(std::memcmp(&est[8 * i], &v[i], 64) == 0);
    CHECK(pts[3] == -1.f && pts[4] == 0.5f && pts[5] == 4.f);
    CHECK(std::fabs(pts[0] - 1.f) < 1e-6f && std::fabs(pts[1] - 2.f) < 1e-6f && std::fabs(pts[2] - 3.f) < 1e-6f);
    if (variant != 2) CHECK(std::fabs(err[3] - 0.0) < 1e-12 && std::fabs(err[7 + 4] - 0.01) < 1e-12);
  }
  std::printf("ok %d\n", n_checks);
  return 0;
}
