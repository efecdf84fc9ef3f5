// orbgpu::MLPnPsolver / orbgpu::mlpnp_collect (include/orbgpu_dropin.hpp) over the mocks of mock_mlpnp.hpp.
//   (no argument)  collect() on a frame that takes every `continue` of the constructor's loop (S/MLPnPsolver.cpp:68-70); prints the
//                  flat problem, then the host half of the library on it: SetRansacParameters' outcome and the minimal sets of a few
//                  raw draws.  Host only.
//   --gpu          the templated solver through iterate(5, ...) in the caller's loop (S/Tracking.cc:3412-3425) on a generated scene;
//                  prints the flat problem, every raw draw the solver took and the outcome of every call with its float bits.
// tests/test_mlpnp_glue.py reads the output.  Compiled with -DMOCK_STRICT_ACCESS as well.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_mlpnp.hpp"
#include "orbgpu_dropin.hpp"

using mock_mlpnp::Camera;
using mock_mlpnp::Frame;
using mock_mlpnp::MapPoint;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void print_f(const char* key, const float* v, size_t n) {
  std::printf("%s:", key);
  for (size_t i = 0; i < n; i++) std::printf(" %08x", bits(v[i]));
  std::printf("\n");
}
template <class T> static void print_i(const char* key, const T* v, size_t n) {
  std::printf("%s:", key);
  for (size_t i = 0; i < n; i++) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}
static void print_flat(const char* tag, const orbgpu::MLPnPFlat& f) {
  std::printf("[%s]\n", tag);
  print_i("m", &f.m, 1);
  print_i("kp_index", f.kp_index.data(), f.kp_index.size());
  print_f("P2D", f.P2D.data(), f.P2D.size());
  print_f("sigma2", f.sigma2.data(), f.sigma2.size());
  print_f("bearing", f.bearing.data(), f.bearing.size());
  print_f("P3Dw", f.P3Dw.data(), f.P3Dw.size());
  print_f("k", f.k, 4);
  print_i("model", &f.model, 1);
}

static int run_collect() {
  Camera cam(0, {500.0f, 400.0f, 320.0f, 240.0f});
  Frame F;
  F.mpCamera = &cam;
  F.TestSetLevels(8, 1.2f);
  const int n_keys = 6, n_matches = 8;             // matches 6 and 7 lie beyond mvKeysUn: the right camera of a rig (:70)
  const int oct[n_keys] = {0, 1, 2, 3, 0, 7};
  for (int i = 0; i < n_keys; i++) F.mvKeysUn.push_back(mock::KeyPoint{{320.0f + 50.0f * i, 240.0f - 40.0f * i}, 31, 0, 0, oct[i]});
  std::vector<std::unique_ptr<MapPoint>> own(n_matches);
  std::vector<MapPoint*> matches(n_matches, nullptr);
  for (int i = 0; i < n_matches; i++) {
    own[i].reset(new MapPoint);
    own[i]->TestSetWorldPos(0.5f * i, -0.25f * i, 4.0f + i);
    matches[i] = own[i].get();
  }
  matches[1] = nullptr;                  // :68 no match
  own[3]->TestSetBad(true);              // :69 bad
  F.mvpMapPoints = matches;
  const orbgpu::MLPnPFlat f = orbgpu::mlpnp_collect<Frame, MapPoint>(F, matches);
  print_flat("collect", f);
  // the host half of the library: SetRansacParameters' formula and the minimal sets
  std::printf("[host]\n");
  for (int n : {6, 7, 19, 21, 100}) {
    int its = 0, mi = 0;
    if (orbp_mlpnp_ransac_iterations(n, 0.99, 10, 300, 6, 0.5f, &its, &mi) != ORBG_OK) return 3;
    const int v[3] = {n, its, mi};
    print_i("n_its_min", v, 3);
  }
  const int32_t draws[12] = {6, 0, 4, 0, 2, 0, 0, 0, 0, 0, 0, 0};
  int32_t idx[12];
  if (orbp_mlpnp_resolve_draws(7, draws, 2, idx) != ORBG_OK) return 3;
  print_i("idx", idx, 12);
  const int32_t bad[6] = {7, 0, 0, 0, 0, 0};
  const int rc = orbp_mlpnp_resolve_draws(7, bad, 1, idx);
  print_i("bad_draw_rc", &rc, 1);
  return 0;
}

struct Lcg {                             // the scene generator of --gpu (not the solver's draws)
  uint64_t s;
  double uni() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
  float range(float a, float b) { return a + (float)uni() * (b - a); }
};

struct RecordingRandomInt {              // DUtils::Random::RandomInt's formula over a private generator; keeps what it handed out
  std::vector<int32_t>* log;
  uint64_t* state;
  int operator()(int min, int max) const {
    *state = *state * 6364136223846793005ULL + 1442695040888963407ULL;
    const int r = (int)((*state >> 33) & 0x7FFFFFFF);
    const int d = max - min + 1;
    const int v = int(((double)r / (2147483647.0 + 1.0)) * d) + min;
    log->push_back(v);
    return v;
  }
};

static int run_gpu() {
  Camera cam(0, {458.654f, 457.296f, 367.215f, 248.375f});
  Frame F;
  F.mpCamera = &cam;
  F.TestSetLevels(8, 1.2f);
  const double c = std::cos(0.3), s = std::sin(0.3);      // the camera: 0.3 rad about y, t = (0.4, -0.1, 0.3)
  const double R[3][3] = {{c, 0, s}, {0, 1, 0}, {-s, 0, c}}, t[3] = {0.4, -0.1, 0.3};
  const int n = 140;
  Lcg g{4321};
  std::vector<std::unique_ptr<MapPoint>> own(n);
  std::vector<MapPoint*> matches(n);
  for (int i = 0; i < n; i++) {
    own[i].reset(new MapPoint);
    const float x = g.range(-2, 2), y = g.range(-1.5f, 1.5f), z = g.range(3, 8);
    own[i]->TestSetWorldPos(x, y, z);
    double pc[3];
    for (int r = 0; r < 3; r++) pc[r] = R[r][0] * x + R[r][1] * y + R[r][2] * z + t[r];
    float u = (float)(458.654 * pc[0] / pc[2] + 367.215) + g.range(-0.5f, 0.5f), v = (float)(457.296 * pc[1] / pc[2] + 248.375) + g.range(-0.5f, 0.5f);
    if (g.uni() < 0.4) { u = g.range(0, 752); v = g.range(0, 480); }      // four matches in ten are wrong
    F.mvKeysUn.push_back(mock::KeyPoint{{u, v}, 31, 0, 0, (int)(g.uni() * 8) & 7});
    matches[i] = i % 13 == 12 ? nullptr : own[i].get();
  }
  own[5]->TestSetBad(true);
  F.mvpMapPoints = matches;
  std::vector<int32_t> log;
  uint64_t state = 77;
  orbgpu::MLPnPsolver<Frame, MapPoint, RecordingRandomInt> solver(F, matches, 0, RecordingRandomInt{&log, &state});
  print_flat("problem", solver.flat());
  std::fflush(stdout);
  solver.SetRansacParameters(0.99, 10, 300, 6, 0.5f, 5.991f);          // S/Tracking.cc:3401
  std::printf("[outcome]\n");
  for (int call = 0; call < 3; call++) {                                // the caller's loop stops at the first matrix; two more calls
    bool bNoMore = false;
    std::vector<bool> vbInliers;
    int nInliers = 0;
    const size_t before = log.size();
    const mock::Mat T = solver.iterate(5, bNoMore, vbInliers, nInliers);
    char key[64];
    const long long flags[4] = {(long long)(log.size() - before), bNoMore, !T.empty(), nInliers};
    std::snprintf(key, sizeof(key), "call%d_draws_nomore_returned_ninliers", call);
    print_i(key, flags, 4);
    std::vector<int> vb(vbInliers.begin(), vbInliers.end());
    std::snprintf(key, sizeof(key), "call%d_vbInliers", call);
    print_i(key, vb.data(), vb.size());
    std::snprintf(key, sizeof(key), "call%d_Tcw", call);
    if (!T.empty()) print_f(key, T.ptr<float>(0), 16);
  }
  print_i("draws", log.data(), log.size());
  return 0;
}

int main(int argc, char** argv) {
  try {
    return argc > 1 && std::strcmp(argv[1], "--gpu") == 0 ? run_gpu() : run_collect();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "glue_mlpnp_check: %s\n", e.what());
    return 2;
  }
}
