// Driver of tests/test_inertial_init_glue.py: the four orbgpu::InertialOptimization overloads (include/orbgpu_inertial.hpp) over the mocks
// of mock_inertial_init.hpp, the library call replaced by a recorder that prints the problem and returns a canned result.
//   argv: overload (1-4), keyframes, and a scenario word:
//     plain     a chain 0 <- 1 <- ... in a map whose maxKFid is the last id
//     beyond    the two newest keyframes lie beyond maxKFid
//     bad       keyframe 2 isBad()
//     missing   keyframe 3's predecessor is not in the list / not in the map's keyframes
//     far       the canned gyro bias lies more than 0.01 from every keyframe's: the Reintegrate() branch
//   then bMono, bFixedVel, priorG (first overload)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mock_inertial_init.hpp"
#include "orbgpu_inertial.hpp"

using namespace mocki;

static bool g_far = false;

struct RecordOps {
  static int information(const float* C, double* i9, double* ig, double* ia) {
    for (int i = 0; i < 81; i++) i9[i] = 0;
    for (int i = 0; i < 9; i++) { ig[i] = 0; ia[i] = 0; }
    i9[0] = C[0];                                            // the edge's own covariance shows in its information
    return ORBG_OK;
  }
  static int solve(const inertial_init_problem& p, inertial_init_result& r) {
    printf("problem size %u algorithm %d iterations %d lambda %g free %d %d %d %d priors %d %g %g bg %g ba %g scale %g Rwg %g %g nk %d ne %d\n",
           p.struct_size == sizeof(p) ? 1u : 0u, p.algorithm, p.iterations, p.lambda_init, p.free_velocity, p.free_bias, p.free_gdir, p.free_scale,
           p.with_priors, p.prior_g, p.prior_a, (double)p.bg[0], (double)p.ba[0], p.scale, p.Rwg[0], p.Rwg[1], p.n_keyframes, p.n_edges);
    for (int k = 0; k < p.n_keyframes; k++) printf("kf %d R0 %g t0 %g v0 %g\n", k, (double)p.keyframes[k].Rwb[0], (double)p.keyframes[k].twb[0], (double)p.keyframes[k].vwb[0]);
    for (int e = 0; e < p.n_edges; e++)
      printf("edge %d k1 %d k2 %d dT %g lbg %g info %g\n", e, p.edges[e].k1, p.edges[e].k2, (double)p.edges[e].preint.dT, (double)p.edges[e].preint.bg[0], p.edges[e].info9[0]);
    for (int k = 0; k < p.n_keyframes; k++) for (int i = 0; i < 3; i++) r.vwb[3 * k + i] = 100.0 + k + 0.25 * i;
    for (int i = 0; i < 3; i++) { r.bg[i] = (g_far ? 0.5 : 0.001) + 0.0001 * i; r.ba[i] = 0.02 + 0.001 * i; }
    for (int i = 0; i < 9; i++) r.Rwg[i] = 0.1 * (i + 1);
    r.scale = 1.75; r.iters = 3;
    mock::log("solve");
    return ORBG_OK;
  }
};

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int overload = atoi(argv[1]), n = atoi(argv[2]);
  const std::string sc = argv[3];
  const bool bMono = argc > 4 ? atoi(argv[4]) != 0 : true, bFixedVel = argc > 5 ? atoi(argv[5]) != 0 : false;
  const float priorG = argc > 6 ? (float)atof(argv[6]) : 1e2f;
  g_far = sc == "far";
  Map map;
  std::vector<KeyFrame> kfs(n);
  std::vector<Preintegrated> pre(n);
  for (int i = 0; i < n; i++) {
    KeyFrame& k = kfs[i];
    k.mnId = 10 + i; k.map = &map;
    Access::R(k).d[0] = 0.5f + i; Access::t(k).d[0] = 1.5f + i; Access::v(k).d[0] = 2.5f + i;
    Access::bias(k) = Bias(0.01f * (i + 1), 0, 0, 0.001f * (i + 1), 0, 0);
    if (i > 0) {
      k.mPrevKF = &kfs[i - 1];
      pre[i].owner = (int)k.mnId; pre[i].dT = 0.1f * i; pre[i].b = Bias(0, 0, 0, 7.f + i, 0, 0); pre[i].C.d[0] = 50.f + i;
      k.mpImuPreintegrated = &pre[i];
    }
  }
  map.max_id = 10 + n - 1 - (sc == "beyond" ? 2 : 0);
  if (sc == "bad") kfs[2].bad = true;
  // the map hands its keyframes over newest first, as a std::set of pointers may; the list overload gets them oldest first
  std::vector<KeyFrame*> list;
  for (int i = n - 1; i >= 0; i--) if (!(sc == "missing" && i == 2)) map.all.push_back(&kfs[i]);
  for (int i = 0; i < n; i++) if (!(sc == "missing" && i == 2)) list.push_back(&kfs[i]);
  Matrix3d Rwg; Vector3d bg, ba; MatrixXd cov; double scale = 1.25;
  Rwg(0, 0) = 0.75; Rwg(0, 1) = -0.25;
  try {
    if (overload == 1) orbgpu::InertialOptimization<RecordOps>(&map, Rwg, scale, bg, ba, bMono, cov, bFixedVel, false, priorG, 1e6f);
    else if (overload == 2) orbgpu::InertialOptimization<RecordOps>(&map, bg, ba, priorG, 1e5f);
    else if (overload == 3) orbgpu::InertialOptimization<RecordOps>(list, bg, ba, priorG, 1e5f);
    else orbgpu::InertialOptimization<RecordOps>(&map, Rwg, scale);
  } catch (const std::exception& ex) {
    printf("threw %s\n", ex.what());
    return 0;
  }
  printf("out scale %g Rwg %g %g bg %g ba %g cov %d\n", scale, Rwg(0, 0), Rwg(2, 2), bg(0), ba(0), cov.touched);
  for (const std::string& e : mock::events()) printf("event %s\n", e.c_str());
  for (int i = 0; i < n; i++) printf("after %lu v %g bwx %g bax %g\n", kfs[i].mnId, (double)Access::v(kfs[i]).d[0], (double)Access::bias(kfs[i]).bwx, (double)Access::bias(kfs[i]).bax);
  return 0;
}
