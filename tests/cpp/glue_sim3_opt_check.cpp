// orbgpu::sim3opt_collect / orbgpu::OptimizeSim3 (include/orbgpu_dropin.hpp) over the mocks of mock_sim3_opt.hpp.
//   (no argument)  the collection loop on a scene that takes every branch of S/Optimizer.cc:4083-4223, with bAllPoints true and
//                  false; prints the scene and the flat problems.  Host only.
//   --gpu          the whole call on a generated scene; prints the scene, the flat problem, g2oS12 before and after with its bits,
//                  which matches were set to NULL, the return value and whether mAcumHessian came back zero.
// tests/test_sim3_opt_cpu.py / tests/test_gpu_sim3_opt.py read the output.  Compiled with -DMOCK_STRICT_ACCESS as well.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_sim3_opt.hpp"
#include "orbgpu_dropin.hpp"

using mock_sim3_opt::KeyFrame;
using mock_sim3_opt::MapPoint;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void print_f(const char* key, const float* v, size_t n) {
  std::printf("%s:", key);
  for (size_t i = 0; i < n; i++) std::printf(" %08x", bits(v[i]));
  std::printf("\n");
}
static void print_d(const char* key, const double* v, size_t n) {
  std::printf("%s:", key);
  for (size_t i = 0; i < n; i++) { uint64_t u; std::memcpy(&u, &v[i], 8); std::printf(" %016llx", (unsigned long long)u); }
  std::printf("\n");
}
template <class T> static void print_i(const char* key, const T* v, size_t n) {
  std::printf("%s:", key);
  for (size_t i = 0; i < n; i++) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}
static void print_flat(const char* tag, const orbgpu::Sim3OptFlat& f) {
  std::printf("[%s]\n", tag);
  print_i("vnIndexEdge", f.vnIndexEdge.data(), f.vnIndexEdge.size());
  const int cnt[5] = {f.nCorrespondences, f.nBadMPs, f.nInKF2, f.nOutKF2, f.nMatchWithoutMP};
  print_i("counters", cnt, 5);
  print_f("X3Dc1", f.X3Dc1.data(), f.X3Dc1.size());
  print_f("X3Dc2", f.X3Dc2.data(), f.X3Dc2.size());
  print_f("obs1", f.obs1.data(), f.obs1.size());
  print_f("obs2", f.obs2.data(), f.obs2.size());
  print_f("w1", f.inv_sigma2_1.data(), f.inv_sigma2_1.size());
  print_f("w2", f.inv_sigma2_2.data(), f.inv_sigma2_2.size());
  print_f("k1", f.k1, 4);
  print_f("k2", f.k2, 4);
}

// A scene in plain arrays, printed for the checker and built into mocks
struct Scene {
  float T1[16], T2[16];
  std::vector<float> keys1, keys2;            // x, y per keypoint
  std::vector<int> oct1, oct2;
  std::vector<int> mp1, match;                // map point id per keypoint of KF1 (-1: none); matched map point id (-1: NULL)
  std::vector<float> pos;                     // 3 per map point
  std::vector<int> bad, idx2, level;          // per map point: isBad, index in KF2 (-1: not observed), mnTrackScaleLevel
  KeyFrame kf1, kf2;
  std::vector<std::unique_ptr<MapPoint>> mps;
  std::vector<MapPoint*> matched;
  void print() const {
    std::printf("[scene]\n");
    print_f("T1", T1, 16); print_f("T2", T2, 16);
    print_f("keys1", keys1.data(), keys1.size()); print_f("keys2", keys2.data(), keys2.size());
    print_i("oct1", oct1.data(), oct1.size()); print_i("oct2", oct2.data(), oct2.size());
    print_i("mp1", mp1.data(), mp1.size()); print_i("match", match.data(), match.size());
    print_f("pos", pos.data(), pos.size());
    print_i("bad", bad.data(), bad.size()); print_i("idx2", idx2.data(), idx2.size()); print_i("level", level.data(), level.size());
    print_f("inv1", kf1.mvInvLevelSigma2.data(), kf1.mvInvLevelSigma2.size());
    print_f("inv2", kf2.mvInvLevelSigma2.data(), kf2.mvInvLevelSigma2.size());
  }
  void build(mock::GeometricCamera* cam1, mock::GeometricCamera* cam2, float sf1, float sf2) {
    kf1.TestSetPose(T1); kf2.TestSetPose(T2);
    kf1.mpCamera = cam1; kf2.mpCamera = cam2;
    kf1.TestSetInvLevels(8, sf1); kf2.TestSetInvLevels(8, sf2);
    for (size_t i = 0; i < oct1.size(); i++) kf1.mvKeysUn.push_back(mock::KeyPoint{{keys1[2 * i], keys1[2 * i + 1]}, 31, 0, 0, oct1[i]});
    for (size_t i = 0; i < oct2.size(); i++) kf2.mvKeysUn.push_back(mock::KeyPoint{{keys2[2 * i], keys2[2 * i + 1]}, 31, 0, 0, oct2[i]});
    for (size_t m = 0; m < bad.size(); m++) {
      mps.emplace_back(new MapPoint);
      mps[m]->TestSetWorldPos(pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
      mps[m]->TestSetBad(bad[m] != 0);
      if (idx2[m] >= 0) mps[m]->TestObserve(&kf2, idx2[m]);
      mps[m]->mnTrackScaleLevel = level[m];
    }
    std::vector<mock_sim3::MapPoint*> own;
    for (size_t i = 0; i < mp1.size(); i++) own.push_back(mp1[i] >= 0 ? mps[mp1[i]].get() : nullptr);
    kf1.TestSetMapPoints(own);
    for (size_t i = 0; i < match.size(); i++) matched.push_back(match[i] >= 0 ? mps[match[i]].get() : nullptr);
  }
};

static int run_collect() {
  mock::GeometricCamera cam1(0, {458.654f, 457.296f, 367.215f, 248.375f}), cam2(0, {435.2f, 435.2f, 320.0f, 240.0f});
  Scene sc;
  const float c = 0.95533649f, s = 0.29552021f;      // cos / sin of 0.3 rad about z
  const float T1[16] = {1, 0, 0, 0.5f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float T2[16] = {c, -s, 0, 0.1f, s, c, 0, -0.2f, 0, 0, 1, 1, 0, 0, 0, 1};
  std::memcpy(sc.T1, T1, sizeof(T1)); std::memcpy(sc.T2, T2, sizeof(T2));
  const int N = 12;
  for (int i = 0; i < N; i++) { sc.keys1.push_back(10.5f * i + 3); sc.keys1.push_back(400 - 7.25f * i); sc.oct1.push_back((3 * i + 1) & 7); }
  for (int i = 0; i < 8; i++) { sc.keys2.push_back(600 - 11.5f * i); sc.keys2.push_back(20 + 9.75f * i); sc.oct2.push_back((5 * i + 2) & 7); }
  // map points 0..11: KF1's own; 12..23: the matched ones
  for (int m = 0; m < 24; m++) {
    sc.pos.push_back(0.3f * (m % 12) - 1.5f + (m >= 12 ? 0.013f : 0)); sc.pos.push_back(1.1f - 0.17f * (m % 12)); sc.pos.push_back(4 + 0.37f * (m % 12));
    sc.bad.push_back(0); sc.idx2.push_back(-1); sc.level.push_back(m % 5);
  }
  for (int i = 0; i < N; i++) { sc.mp1.push_back(i); sc.match.push_back(12 + i); }
  sc.idx2[12 + 0] = 0;                                   // 0: kept, seen in KF2
  sc.match[1] = -1;                                      // 1: vpMatches1[i] == NULL (:4085)
  sc.bad[2] = 1; sc.idx2[12 + 2] = 1;                    // 2: bad pMP1 (:4104)
  sc.bad[12 + 3] = 1; sc.idx2[12 + 3] = 2;               // 3: bad pMP2 (:4104)
  sc.mp1[4] = -1; sc.idx2[12 + 4] = 4;                   // 4: pMP1 == NULL (:4128)
  sc.mp1[5] = -1; sc.bad[12 + 5] = 1;                    // 5: pMP1 == NULL and pMP2 bad (:4133)
  /* 6: i2 < 0 (:4148 with bAllPoints false; :4192-4210 with true) */
  sc.pos[3 * (12 + 7) + 2] = -3.0f; sc.idx2[12 + 7] = 6; // 7: z < 0 in KF2 (:4154)
  sc.idx2[12 + 8] = 3;                                   // 8: kept, seen in KF2
  sc.pos[3 * (12 + 9) + 2] = -2.5f;                      // 9: i2 < 0 and z < 0
  sc.idx2[12 + 10] = 5;                                  // 10: kept
  sc.match[11] = -1;                                     // 11: NULL
  sc.build(&cam1, &cam2, 1.2f, 1.5f);
  sc.print();
  print_flat("all_points", orbgpu::sim3opt_collect<KeyFrame, MapPoint>(&sc.kf1, &sc.kf2, sc.matched, true));
  print_flat("only_in_kf2", orbgpu::sim3opt_collect<KeyFrame, MapPoint>(&sc.kf1, &sc.kf2, sc.matched, false));
  return 0;
}

struct Lcg {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
  float range(float a, float b) { return a + (float)uni() * (b - a); }
};

static int run_gpu() {
  mock::GeometricCamera cam1(0, {458.654f, 457.296f, 367.215f, 248.375f}), cam2(0, {435.2f, 435.2f, 320.0f, 240.0f});
  Scene sc;
  const float c = 0.98006658f, s = 0.19866933f;      // cos / sin of 0.2 rad about y
  const float T1[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float T2[16] = {c, 0, s, 0.4f, 0, 1, 0, -0.1f, -s, 0, c, 0.3f, 0, 0, 0, 1};
  std::memcpy(sc.T1, T1, sizeof(T1)); std::memcpy(sc.T2, T2, sizeof(T2));
  const int N = 180;
  Lcg g{4711};
  const float* K1 = nullptr; (void)K1;
  for (int i = 0; i < N; i++) {
    // one world point seen by both keyframes; KF1's map holds it as point i, the other map as point N + i (a centimetre away, or
    // somewhere else entirely for one match in four)
    const float x = g.range(-2, 2), y = g.range(-1.5f, 1.5f), z = g.range(4, 10);
    sc.pos.push_back(x); sc.pos.push_back(y); sc.pos.push_back(z);
    sc.bad.push_back(0); sc.idx2.push_back(-1); sc.level.push_back(0);
    sc.mp1.push_back(i % 17 == 16 ? -1 : i);
    sc.match.push_back(i % 13 == 12 ? -1 : N + i);
    sc.oct1.push_back((int)(g.uni() * 8) & 7);
    // KF1 observes it where it projects (T1 = identity), plus half a pixel
    sc.keys1.push_back(458.654f * x / z + 367.215f + g.range(-0.5f, 0.5f)); sc.keys1.push_back(457.296f * y / z + 248.375f + g.range(-0.5f, 0.5f));
  }
  for (int i = 0; i < N; i++) {
    const bool wrong = g.uni() < 0.25;
    const float x = wrong ? g.range(-2, 2) : sc.pos[3 * i] + g.range(-0.01f, 0.01f);
    const float y = wrong ? g.range(-1.5f, 1.5f) : sc.pos[3 * i + 1] + g.range(-0.01f, 0.01f);
    const float z = wrong ? g.range(4, 10) : sc.pos[3 * i + 2] + g.range(-0.01f, 0.01f);
    sc.pos.push_back(x); sc.pos.push_back(y); sc.pos.push_back(z);
    sc.bad.push_back(i % 29 == 28 ? 1 : 0); sc.level.push_back(i % 7);
    const bool in2 = i % 6 != 5;
    sc.idx2.push_back(in2 ? i : -1);
    // KF2's keypoint i: the projection of the matched point through T2, plus half a pixel
    const float xc = c * x + s * z + 0.4f, yc = y - 0.1f, zc = -s * x + c * z + 0.3f;
    sc.keys2.push_back(435.2f * xc / zc + 320.0f + g.range(-0.5f, 0.5f)); sc.keys2.push_back(435.2f * yc / zc + 240.0f + g.range(-0.5f, 0.5f));
    sc.oct2.push_back((int)(g.uni() * 8) & 7);
  }
  sc.build(&cam1, &cam2, 1.2f, 1.2f);
  sc.print();
  // S12 maps camera-2 coordinates to camera-1 coordinates: the inverse of T2 here, disturbed
  const double th = -0.2 + 0.004;
  mock_sim3_opt::Sim3 S12(mock_sim3_opt::Quaterniond(std::cos(th / 2), 0.001, std::sin(th / 2), -0.0015),
                          mock_sim3_opt::Vector3d(-(c * 0.4 - s * 0.3) + 0.01, 0.1 - 0.008, -(s * 0.4 + c * 0.3) + 0.012), 1.0);
  for (int pass = 0; pass < 2; pass++) {
    const bool all_points = pass == 0;
    std::vector<MapPoint*> vp = sc.matched;
    mock_sim3_opt::Sim3 S = S12;
    mock_sim3_opt::Matrix7d Hs;
    for (int k = 0; k < 49; k++) Hs.m[k] = 3.25;
    print_flat(all_points ? "problem_all" : "problem_kf2", orbgpu::sim3opt_collect<KeyFrame, MapPoint>(&sc.kf1, &sc.kf2, vp, all_points));
    std::fflush(stdout);
    const int nIn = orbgpu::OptimizeSim3<KeyFrame, MapPoint>(&sc.kf1, &sc.kf2, vp, S, 10.0f, pass == 0, Hs, all_points);
    std::printf("[%s]\n", all_points ? "outcome_all" : "outcome_kf2");
    const double in[8] = {S12.rotation().coeffs()[0], S12.rotation().coeffs()[1], S12.rotation().coeffs()[2], S12.rotation().coeffs()[3],
                          S12.translation()[0], S12.translation()[1], S12.translation()[2], S12.scale()};
    const double out[8] = {S.rotation().coeffs()[0], S.rotation().coeffs()[1], S.rotation().coeffs()[2], S.rotation().coeffs()[3],
                           S.translation()[0], S.translation()[1], S.translation()[2], S.scale()};
    print_d("S12_in", in, 8); print_d("S12_out", out, 8);
    std::vector<int> null_now;
    for (size_t i = 0; i < vp.size(); i++) null_now.push_back(vp[i] == nullptr ? 1 : 0);
    print_i("null", null_now.data(), null_now.size());
    bool zero = true;
    for (int k = 0; k < 49; k++) zero = zero && Hs.m[k] == 0.0;
    const int ret[3] = {nIn, zero ? 1 : 0, pass == 0 ? 1 : 0};
    print_i("nIn_hessianzero_fixscale", ret, 3);
  }
  return 0;
}

int main(int argc, char** argv) {
  try {
    return argc > 1 && std::strcmp(argv[1], "--gpu") == 0 ? run_gpu() : run_collect();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "glue_sim3_opt_check: %s\n", e.what());
    return 2;
  }
}
