// orbgpu::CreateNewMapPoints (include/orbgpu_localmapping.hpp) over liborbgpu against the serial restatement of new_points_ref.hpp,
// each on its own copy of the same mock map (mock_newpoints.hpp).
//   --gpu [stop_after]   a stereo and a monocular-inertial scene (neighbours the baseline gates leave out, an mPrevKF chain, features
//                        that already hold points); CheckNewKeyFrames() turns true at its stop_after-th call (0: never).  Prints per
//                        scene the created points of both sides -- neighbour keyframe, idx1, idx2, the position's float bits -- and
//                        what the keyframes hold afterwards.  tests/test_newpoints_glue.py compares.
//   --time n B mono reps the restatement timed on one scene (median of reps, microseconds; no device needed).
// Compiled with -DMOCK_STRICT_ACCESS: the glue stays within what the reference's classes let an outsider touch.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_newpoints.hpp"
#include "new_points_ref.hpp"
#include "orbgpu_localmapping.hpp"

using mock_np::KeyFrame;
using mock_np::MapPoint;

struct Lcg {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
  double range(double a, double b) { return a + uni() * (b - a); }
  double normal() { double t = 0; for (int i = 0; i < 12; i++) t += uni(); return t - 6.0; }
  int below(int n) { return (int)(uni() * n) % n; }
};

struct World {                    // one copy of the map
  mock::GeometricCamera cam{0, {458.f, 457.f, 367.f, 248.f}};
  std::vector<std::unique_ptr<KeyFrame>> kfs;          // [0] = the current keyframe
  std::vector<std::unique_ptr<MapPoint>> points;
  std::vector<MapPoint*> created;
};

static void rot_y(double a, double yaw_x, float* T12, const double* C) {      // Rcw = Ry(a) Rx(yaw_x), tcw = -Rcw C
  const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(yaw_x), sb = std::sin(yaw_x);
  const double R[9] = {ca, sa * sb, sa * cb, 0, cb, -sb, -sa, ca * sb, ca * cb};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T12[4 * i + j] = (float)R[3 * i + j];
    T12[4 * i + 3] = (float)-(R[3 * i] * C[0] + R[3 * i + 1] * C[1] + R[3 * i + 2] * C[2]);
  }
}

// n features per keyframe, nkf neighbours; the same seed gives the same map.  Neighbour 1 sits closer than mb (the stereo baseline
// gate), neighbour 2 has a huge median depth (the monocular gate).
static void build(World& w, uint64_t seed, int n, int nkf, bool mono, bool chain) {
  Lcg g{seed};
  const int n_nodes = std::max(4, n / 8);
  std::vector<double> X((size_t)3 * n);
  std::vector<int> node(n), octave(n);
  std::vector<std::vector<uint8_t>> centre(n_nodes, std::vector<uint8_t>(32)), base(n, std::vector<uint8_t>(32));
  for (auto& c : centre) for (auto& b : c) b = (uint8_t)g.below(256);
  for (int i = 0; i < n; i++) {
    const double z = g.range(2, 12), u = g.range(20, 730), v = g.range(20, 470);
    X[3 * i] = (u - 367) / 458 * z; X[3 * i + 1] = (v - 248) / 457 * z; X[3 * i + 2] = z;
    node[i] = g.below(n_nodes) * 5 + 2; octave[i] = g.below(8);
    base[i] = centre[(node[i] - 2) / 5];
    for (int f = 0; f < 18; f++) { const int bit = g.below(256); base[i][bit >> 3] ^= (uint8_t)(1 << (bit & 7)); }
  }
  for (int k = 0; k <= nkf; k++) {
    std::unique_ptr<KeyFrame> kf(new KeyFrame);
    double C[3] = {0, 0, 0};
    if (k > 0) {
      const double len = (k == 2 && !mono) ? 0.05 : g.range(0.15, 0.5), ang = g.range(0, 6.28);
      C[0] = len * std::cos(ang); C[1] = len * std::sin(ang) * 0.6; C[2] = g.range(-0.05, 0.05);
    }
    float T12[12];
    rot_y(k == 0 ? 0.0 : g.range(-0.05, 0.05), k == 0 ? 0.0 : g.range(-0.03, 0.03), T12, C);
    kf->TestSetPose(T12);
    kf->TestSetLevels(8, 1.2f);
    kf->mpCamera = &w.cam;
    kf->fx = 458.f; kf->fy = 457.f; kf->cx = 367.f; kf->cy = 248.f; kf->invfx = 1.0f / kf->fx; kf->invfy = 1.0f / kf->fy;
    kf->mb = 0.11f; kf->mbf = kf->mb * kf->fx;
    kf->N = n;
    kf->mDescriptors = mock::Mat(n, 32, 1);
    if (k == 3 && mono) kf->test_median_depth = 1e4f;
    std::vector<int> perm(n);
    for (int i = 0; i < n; i++) perm[i] = i;
    if (k > 0) for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[g.below(i + 1)]);
    std::vector<MapPoint*> mps(n, nullptr);
    for (int j = 0; j < n; j++) {
      const int i = perm[j];
      const double xc = T12[0] * X[3 * i] + T12[1] * X[3 * i + 1] + T12[2] * X[3 * i + 2] + T12[3];
      const double yc = T12[4] * X[3 * i] + T12[5] * X[3 * i + 1] + T12[6] * X[3 * i + 2] + T12[7];
      const double zc = T12[8] * X[3 * i] + T12[9] * X[3 * i + 1] + T12[10] * X[3 * i + 2] + T12[11];
      const int oct = std::min(7, std::max(0, octave[i] + (g.uni() < 0.2 ? g.below(3) - 1 : 0)));
      const double s = kf->mvScaleFactors[oct];
      float u = (float)(458 * xc / zc + 367 + g.normal() * s), v = (float)(457 * yc / zc + 248 + g.normal() * s);
      if (k > 0 && g.uni() < 0.15) { u = (float)g.range(20, 730); v = (float)g.range(20, 470); }    // gross mismatch
      const mock::KeyPoint kp{{u, v}, (float)(31 * s), (float)g.range(0, 360), 0.f, oct};
      kf->mvKeys.push_back(kp); kf->mvKeysUn.push_back(kp);
      const bool stereo = !mono && g.uni() < 0.5;
      kf->mvDepth.push_back(stereo ? (float)zc : -1.f);
      kf->mvuRight.push_back(stereo ? (float)(u - kf->mbf / zc) : -1.f);
      std::vector<uint8_t> d = base[i];
      for (int f = g.below(7); f > 0; f--) { const int bit = g.below(256); d[bit >> 3] ^= (uint8_t)(1 << (bit & 7)); }
      std::memcpy(kf->mDescriptors.ptr<uint8_t>(j), d.data(), 32);
      kf->mFeatVec[(unsigned)(g.uni() < 0.05 ? g.below(n_nodes + 2) * 5 + 2 : node[i])].push_back((unsigned)j);
      if (g.uni() < 0.2) {
        mock::Mat P(3, 1, 4);
        w.points.emplace_back(new MapPoint(P, kf.get()));
        mps[j] = w.points.back().get();
      }
    }
    kf->TestSetMapPoints(mps);
    w.kfs.push_back(std::move(kf));
  }
  std::vector<KeyFrame*> nb;
  const int listed = chain ? nkf - 2 : nkf;                                   // the last two neighbours come in through the mPrevKF chain
  for (int k = 1; k <= listed; k++) nb.push_back(w.kfs[k].get());
  w.kfs[0]->TestSetNeighbours(nb);
  if (chain) { w.kfs[0]->mPrevKF = w.kfs[nkf - 1].get(); w.kfs[nkf - 1]->mPrevKF = w.kfs[1].get(); w.kfs[1]->mPrevKF = w.kfs[nkf].get(); }
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void dump(const char* tag, const World& w) {
  std::printf("[%s]\n", tag);
  for (MapPoint* p : w.created) {
    int kf2 = -1, idx1 = -1, idx2 = -1;
    for (const auto& ob : p->TestObservations())
      for (size_t k = 0; k < w.kfs.size(); k++)
        if (w.kfs[k].get() == ob.first) { if (k == 0) idx1 = ob.second; else { kf2 = (int)k; idx2 = ob.second; } }
    const mock::Mat X = p->GetWorldPos();
    std::printf("point: %d %d %d %08x %08x %08x %d %d %d %d\n", kf2, idx1, idx2, bits(X.ptr<float>(0)[0]), bits(X.ptr<float>(1)[0]), bits(X.ptr<float>(2)[0]),
                p->n_distinctive, p->n_normal_updates, (int)p->TestObservations().size(), p->TestRefKF() == w.kfs[0].get());
  }
  for (size_t k = 0; k < w.kfs.size(); k++) {
    const auto mps = w.kfs[k]->GetMapPointMatches();
    std::printf("kf%zu:", k);
    for (size_t i = 0; i < mps.size(); i++) {
      int c = -1;
      for (size_t q = 0; q < w.created.size(); q++) if (w.created[q] == mps[i]) c = (int)q;
      if (c >= 0) std::printf(" %zu=%d", i, c);
    }
    std::printf("\n");
  }
}

struct StopAt {                   // CheckNewKeyFrames(): true from its k-th call on (0: never)
  int k, calls = 0;
  bool operator()() { calls++; return k > 0 && calls >= k; }
};

static int run_scene(const char* name, uint64_t seed, int n, int nkf, bool mono, bool inertial, int stop_after) {
  World a, b;
  build(a, seed, n, nkf, mono, inertial);
  build(b, seed, n, nkf, mono, inertial);
  auto hooks = [](World& w) {
    return std::make_pair([&w](const mock::Mat& x3D, KeyFrame* ref) { w.points.emplace_back(new MapPoint(x3D, ref)); return w.points.back().get(); },
                          [&w](MapPoint* p) { w.created.push_back(p); });
  };
  auto ha = hooks(a);
  auto hb = hooks(b);
  StopAt sa{stop_after}, sb{stop_after};
  orbgpu::KeyFramesOnDevice<KeyFrame> dev;
  const int made_a = orbgpu::CreateNewMapPoints<mock::Mat>(a.kfs[0].get(), dev, mono, inertial, false, true, 11.5f, std::ref(sa), ha.first, ha.second);
  const int made_b = np_ref::CreateNewMapPoints<mock::Mat>(b.kfs[0].get(), mono, inertial, false, true, 11.5f, std::ref(sb), hb.first, hb.second);
  std::printf("[%s]\nmade: %d %d\ncheck_calls: %d %d\nresident: %zu\n", name, made_a, made_b, sa.calls, sb.calls, dev.size());
  char tag[64];
  std::snprintf(tag, sizeof tag, "%s.glue", name); dump(tag, a);
  std::snprintf(tag, sizeof tag, "%s.ref", name); dump(tag, b);
  // a keyframe of a rig is out of scope: nothing is touched
  World c;
  build(c, seed, 40, 3, mono, false);
  c.kfs[2]->NLeft = 20;
  auto hc = hooks(c);
  StopAt sc{0};
  std::printf("[%s.rig]\nmade: %d %zu %d\n", name, orbgpu::CreateNewMapPoints<mock::Mat>(c.kfs[0].get(), dev, mono, false, false, false, 0.f, std::ref(sc), hc.first, hc.second),
              c.created.size(), sc.calls);
  return 0;
}

static int run_time(int n, int B, bool mono, int reps) {
  std::vector<double> us;
  int made = 0;
  for (int r = 0; r < reps; r++) {
    World w;
    build(w, 77, n, B, mono, false);
    auto NewMP = [&w](const mock::Mat& x3D, KeyFrame* ref) { w.points.emplace_back(new MapPoint(x3D, ref)); return w.points.back().get(); };
    auto Add = [&w](MapPoint* p) { w.created.push_back(p); };
    StopAt s{0};
    const auto t0 = std::chrono::steady_clock::now();
    made = np_ref::CreateNewMapPoints<mock::Mat>(w.kfs[0].get(), mono, false, false, false, 0.f, std::ref(s), NewMP, Add);
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(us.begin(), us.end());
  std::printf("restatement_us: %.1f\nmade: %d\n", us[us.size() / 2], made);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 6 && std::strcmp(argv[1], "--time") == 0) return run_time(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) != 0, std::atoi(argv[5]));
    if (argc >= 2 && std::strcmp(argv[1], "--gpu") == 0) {
      const int stop_after = argc >= 3 ? std::atoi(argv[2]) : 0;
      run_scene("stereo", 11, 180, 6, false, false, stop_after);
      run_scene("mono_inertial", 12, 150, 7, true, true, stop_after);
      return 0;
    }
    std::fprintf(stderr, "usage: new_points_glue --gpu [stop_after] | --time n B mono reps\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "new_points_glue: %s\n", e.what());
    return 2;
  }
}
