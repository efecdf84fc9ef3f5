// orbgpu::Sim3Solver / orbgpu::sim3_collect (include/orbgpu_dropin.hpp) over the mocks of mock_sim3.hpp.
//   (no argument)  collect() on a scene that takes every `continue` of the constructor's loop (S/Sim3Solver.cc:79-97), with and
//                  without vpKeyFrameMatchedMP; prints the flat problem.  Host only.
//   --gpu          the templated solver through iterate(20, ...) in the caller's loop (S/LoopClosing.cc:715-718) on a generated scene;
//                  prints the flat problem, every raw draw the solver took and the outcome with its float bits.
// tests/test_sim3_cpu.py / tests/test_gpu_sim3.py read the output.  Compiled with -DMOCK_STRICT_ACCESS as well.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_sim3.hpp"
#include "orbgpu_dropin.hpp"

using mock_sim3::KeyFrame;
using mock_sim3::MapPoint;

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
static void print_flat(const char* tag, const orbgpu::Sim3Flat& f) {
  std::printf("[%s]\n", tag);
  print_i("mN1", &f.mN1, 1);
  print_i("indices1", f.indices1.data(), f.indices1.size());
  print_i("max_err1", f.max_err1.data(), f.max_err1.size());
  print_i("max_err2", f.max_err2.data(), f.max_err2.size());
  print_f("X3Dc1", f.X3Dc1.data(), f.X3Dc1.size());
  print_f("X3Dc2", f.X3Dc2.data(), f.X3Dc2.size());
  print_f("k1", f.k1, 4);
  print_f("k2", f.k2, 4);
  const int fs = f.fix_scale;
  print_i("fix_scale", &fs, 1);
}

static int run_collect() {
  mock::GeometricCamera cam1(0, {458.654f, 457.296f, 367.215f, 248.375f}), cam2(0, {435.2f, 435.2f, 320.0f, 240.0f});
  KeyFrame kf1, kf2, kf3;
  const float T1[16] = {1, 0, 0, 0.5f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float T2[16] = {0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1};
  kf1.TestSetPose(T1); kf2.TestSetPose(T2); kf3.TestSetPose(T1);
  kf1.mpCamera = &cam1; kf2.mpCamera = &cam2; kf3.mpCamera = &cam1;
  kf1.TestSetLevels(8, 1.2f); kf2.TestSetLevels(8, 1.2f); kf3.TestSetLevels(8, 2.0f);
  const int n = 8;
  const int oct1[n] = {1, 0, 0, 0, 0, 0, 0, 3}, oct2[n] = {0, 0, 0, 0, 0, 0, 0, 7};
  for (int i = 0; i < n; i++) {
    kf1.mvKeysUn.push_back(mock::KeyPoint{{0, 0}, 31, 0, 0, oct1[i]});
    kf2.mvKeysUn.push_back(mock::KeyPoint{{0, 0}, 31, 0, 0, oct2[i]});
    kf3.mvKeysUn.push_back(mock::KeyPoint{{0, 0}, 31, 0, 0, 5});
  }
  std::vector<std::unique_ptr<MapPoint>> own(n), other(n);
  std::vector<MapPoint*> mp1(n, nullptr), matched(n, nullptr);
  for (int i = 0; i < n; i++) {
    own[i].reset(new MapPoint); other[i].reset(new MapPoint);
    own[i]->TestSetWorldPos(1, 2, 5); other[i]->TestSetWorldPos(1, 2, 5.25f);
    own[i]->TestObserve(&kf1, i); other[i]->TestObserve(&kf2, i); other[i]->TestObserve(&kf3, i);
    mp1[i] = own[i].get(); matched[i] = other[i].get();
  }
  own[7]->TestSetWorldPos(-1, 0.5f, 4); other[7]->TestSetWorldPos(-1, 0.5f, 4);
  matched[1] = nullptr;                  // :79   no match
  mp1[2] = nullptr;                      // :84   the keyframe has no point of its own there
  own[3]->TestSetBad(true);              // :87   bad on side 1
  other[4]->TestSetBad(true);            // :87   bad on side 2
  own[5].reset(new MapPoint); own[5]->TestSetWorldPos(1, 2, 5); mp1[5] = own[5].get();          // :96 not observed by pKF1
  other[6].reset(new MapPoint); other[6]->TestSetWorldPos(1, 2, 5.25f); matched[6] = other[6].get();   // :96 not observed by pKF2
  kf1.TestSetMapPoints(mp1);
  print_flat("default", orbgpu::sim3_collect<KeyFrame, MapPoint>(&kf1, &kf2, matched, true));
  // the caller names another keyframe (other levels, octave 5 everywhere) for every matched point: the constructor never reads it
  print_flat("with_keyframes", orbgpu::sim3_collect<KeyFrame, MapPoint>(&kf1, &kf2, matched, false, std::vector<KeyFrame*>(n, &kf3)));
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
  mock::GeometricCamera cam1(0, {458.654f, 457.296f, 367.215f, 248.375f}), cam2(0, {435.2f, 435.2f, 320.0f, 240.0f});
  KeyFrame kf1, kf2;
  const float c = 0.95533649f, s = 0.29552021f;      // cos / sin of 0.3 rad about y
  const float T1[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float T2[16] = {c, 0, s, 0.4f, 0, 1, 0, -0.1f, -s, 0, c, 0.3f, 0, 0, 0, 1};
  kf1.TestSetPose(T1); kf2.TestSetPose(T2);
  kf1.mpCamera = &cam1; kf2.mpCamera = &cam2;
  kf1.TestSetLevels(8, 1.2f); kf2.TestSetLevels(8, 1.2f);
  const int n = 150;
  Lcg g{12345};
  std::vector<std::unique_ptr<MapPoint>> own(n), other(n);
  std::vector<MapPoint*> mp1(n), matched(n);
  for (int i = 0; i < n; i++) {
    kf1.mvKeysUn.push_back(mock::KeyPoint{{0, 0}, 31, 0, 0, (int)(g.uni() * 8) & 7});
    kf2.mvKeysUn.push_back(mock::KeyPoint{{0, 0}, 31, 0, 0, (int)(g.uni() * 8) & 7});
    own[i].reset(new MapPoint); other[i].reset(new MapPoint);
    const float x = g.range(-3, 3), y = g.range(-2, 2), z = g.range(3, 10);
    own[i]->TestSetWorldPos(x, y, z);
    // the other map's point: the same place plus a centimetre of noise, or somewhere else entirely for seven matches in ten
    if (g.uni() < 0.7) other[i]->TestSetWorldPos(g.range(-3, 3), g.range(-2, 2), g.range(3, 10));
    else other[i]->TestSetWorldPos(x + g.range(-0.01f, 0.01f), y + g.range(-0.01f, 0.01f), z + g.range(-0.01f, 0.01f));
    own[i]->TestObserve(&kf1, i); other[i]->TestObserve(&kf2, i);
    mp1[i] = own[i].get(); matched[i] = i % 11 == 10 ? nullptr : other[i].get();
  }
  kf1.TestSetMapPoints(mp1);
  print_flat("problem", orbgpu::sim3_collect<KeyFrame, MapPoint>(&kf1, &kf2, matched, true));
  std::fflush(stdout);
  std::vector<int32_t> log;
  uint64_t state = 99;
  orbgpu::Sim3Solver<KeyFrame, MapPoint, RecordingRandomInt> solver(&kf1, &kf2, matched, true, std::vector<KeyFrame*>(), 0,
                                                                    RecordingRandomInt{&log, &state});
  solver.SetRansacParameters(0.99, 25, 300);
  bool bNoMore = false, bConverge = false;
  std::vector<bool> vbInliers;
  int nInliers = 0, calls = 0;
  mock::Mat T;
  while (!bConverge && !bNoMore) {                   // S/LoopClosing.cc:715-718
    T = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
    calls++;
  }
  std::printf("[outcome]\n");
  print_i("draws", log.data(), log.size());
  const int flags[4] = {calls, bNoMore, bConverge, nInliers};
  print_i("calls_nomore_converge_ninliers", flags, 4);
  std::vector<int> vb(vbInliers.begin(), vbInliers.end());
  print_i("vbInliers", vb.data(), vb.size());
  if (!T.empty()) print_f("T12", T.ptr<float>(0), 16);
  const mock::Mat R = solver.GetEstimatedRotation(), t = solver.GetEstimatedTranslation();
  if (!R.empty()) { print_f("R", R.ptr<float>(0), 9); print_f("t", t.ptr<float>(0), 3); }
  const float sc = solver.GetEstimatedScale();
  print_f("s", &sc, 1);
  return 0;
}

int main(int argc, char** argv) {
  try {
    return argc > 1 && std::strcmp(argv[1], "--gpu") == 0 ? run_gpu() : run_collect();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "glue_sim3_check: %s\n", e.what());
    return 2;
  }
}
