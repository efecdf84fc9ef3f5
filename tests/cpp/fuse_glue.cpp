// orbgpu::SearchInNeighbors / orbgpu::Fuse (include/orbgpu_localmapping.hpp) over liborbgpu against the serial restatement of
// fuse_ref.hpp, each on its own copy of the same mock map (mock_fuse.hpp).
//   --gpu [abort_after]   a stereo and a monocular-inertial scene: second neighbours that repeat (and name the current keyframe), a
//                         bad keyframe, an mPrevKF chain, map points shared between keyframes and duplicates of them, so that points
//                         are replaced in one target and met again -- with another descriptor -- in a later one; mbAbortBA turns
//                         true at its abort_after-th reading (0: never).  Prints per scene and side every keyframe's point table
//                         and marks, every point's state, the return values; then a stand-alone Fuse call and a rig scene.
//                         tests/test_fuse_glue.py compares.
//   --time n targets mono reps   SearchInNeighbors at n features per keyframe: the glue and the restatement, median of reps
//                         (microseconds), each repetition on a fresh copy of the map; the glue's keyframes are resident (uploaded
//                         by an untimed first call on another copy).
// Compiled with -DMOCK_STRICT_ACCESS: the glue stays within what the reference's classes let an outsider touch (+ edit E1).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "mock_fuse.hpp"
#include "fuse_ref.hpp"
#include "orbgpu_localmapping.hpp"

using mock_fuse::KeyFrame;
using mock_fuse::MapPoint;

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
};

static void pose(double a, double b, float* T12, const double* C) {      // Rcw = Ry(a) Rx(b), tcw = -Rcw C
  const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b);
  const double R[9] = {ca, sa * sb, sa * cb, 0, cb, -sb, -sa, ca * sb, ca * cb};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T12[4 * i + j] = (float)R[3 * i + j];
    T12[4 * i + 3] = (float)-(R[3 * i] * C[0] + R[3 * i + 1] * C[1] + R[3 * i + 2] * C[2]);
  }
}

// nkf keyframes of n features over n world points; a world point has one map point and, one time in two, a duplicate of it (what
// another keyframe's CreateNewMapPoints would have made).  A feature holds the point, its duplicate or nothing.  The same seed gives
// the same map.  listed: how many keyframes the current one names as covisible; chain: the others hang on the mPrevKF chain.
// World point 0 is the crowded case: the current keyframe holds its point, the first target its duplicate on a feature with the
// point's own descriptor, the second target nothing, and every target has `crowd` more features of the right level within 1.5 px of
// it -- so the point survives a Replace in the first target, gets a new descriptor, and meets more candidates than a record lists
// in the second one.
static void build(World& w, uint64_t seed, int n, int nkf, int listed, bool mono, bool chain, int crowd = 0) {
  Lcg g{seed};
  std::vector<double> X((size_t)3 * n);
  std::vector<int> level(n);
  std::vector<std::vector<uint8_t>> base(n, std::vector<uint8_t>(32));
  std::vector<MapPoint*> first(n), second(n, nullptr);
  const double sf = 1.2;
  for (int i = 0; i < n; i++) {
    const double z = g.range(2, 12), u = g.range(20, 730), v = g.range(20, 470);
    X[3 * i] = (u - 367) / 458 * z; X[3 * i + 1] = (v - 248) / 457 * z; X[3 * i + 2] = z;
    level[i] = g.below(8);
    for (auto& b : base[i]) b = (uint8_t)g.below(256);
    const double d = std::sqrt(X[3 * i] * X[3 * i] + X[3 * i + 1] * X[3 * i + 1] + z * z);
    for (int c = 0; c < 2; c++) {
      if (c == 1 && g.uni() < 0.5 && i != 0) continue;
      const float Xf[3] = {(float)(X[3 * i] + g.normal() * 0.002), (float)(X[3 * i + 1] + g.normal() * 0.002), (float)(z + g.normal() * 0.004)};
      float nv[3] = {(float)(X[3 * i] / d), (float)(X[3 * i + 1] / d), (float)(z / d)};
      if (g.uni() < 0.05) nv[2] = -nv[2];                                          // seen from behind: the normal gate (not world point 0, below)
      float maxd = (float)(d * std::pow(sf, level[i] + g.range(-0.4, 0.4)) * (g.uni() < 0.05 ? 0.4 : 1.0));
      if (i == 0) { nv[2] = (float)(z / d); maxd = (float)(d * std::pow(sf, level[i] - 0.3)); }
      std::vector<uint8_t> dsc = base[i];
      for (int f = g.below(10); f > 0; f--) { const int bit = g.below(256); dsc[bit >> 3] ^= (uint8_t)(1 << (bit & 7)); }
      w.points.emplace_back(new MapPoint(w.points.size() + 1, Xf, nv, (float)(maxd / std::pow(sf, 7)), maxd, dsc.data()));
      (c == 0 ? first[i] : second[i]) = w.points.back().get();
    }
  }
  for (int k = 0; k <= nkf; k++) {
    std::unique_ptr<KeyFrame> kf(new KeyFrame);
    kf->mnId = 100 + k;
    double C[3] = {0, 0, 0};
    if (k > 0) { const double len = g.range(0.15, 0.5), ang = g.range(0, 6.28); C[0] = len * std::cos(ang); C[1] = len * std::sin(ang) * 0.6; C[2] = g.range(-0.05, 0.05); }
    float T12[12];
    pose(k == 0 ? 0.0 : g.range(-0.05, 0.05), k == 0 ? 0.0 : g.range(-0.03, 0.03), T12, C);
    kf->TestSetPose(T12);
    kf->TestSetLevels(8, 1.2f);
    kf->mpCamera = &w.cam;
    kf->fx = 458.f; kf->fy = 457.f; kf->cx = 367.f; kf->cy = 248.f; kf->invfx = 1.0f / kf->fx; kf->invfy = 1.0f / kf->fy;
    kf->mb = 0.11f; kf->mbf = kf->mb * kf->fx;
    kf->N = n;
    kf->mDescriptors = mock::Mat(n, 32, 1);
    std::vector<int> perm(n);
    for (int i = 0; i < n; i++) perm[i] = i;
    for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[g.below(i + 1)]);
    std::vector<MapPoint*> mps(n, nullptr);
    std::vector<std::pair<MapPoint*, int>> held;
    const double z0 = T12[8] * X[0] + T12[9] * X[1] + T12[10] * X[2] + T12[11];      // where this keyframe sees world point 0
    const double u0 = 458 * (T12[0] * X[0] + T12[1] * X[1] + T12[2] * X[2] + T12[3]) / z0 + 367, v0 = 457 * (T12[4] * X[0] + T12[5] * X[1] + T12[6] * X[2] + T12[7]) / z0 + 248;
    for (int j = 0; j < n; j++) {
      const int i = perm[j];
      const double xc = T12[0] * X[3 * i] + T12[1] * X[3 * i + 1] + T12[2] * X[3 * i + 2] + T12[3];
      const double yc = T12[4] * X[3 * i] + T12[5] * X[3 * i + 1] + T12[6] * X[3 * i + 2] + T12[7];
      const double zc = T12[8] * X[3 * i] + T12[9] * X[3 * i + 1] + T12[10] * X[3 * i + 2] + T12[11];
      int oct = std::min(7, std::max(0, level[i] - (g.uni() < 0.5 ? 1 : 0)));
      if (g.uni() < 0.08) oct = std::min(7, oct + 2);                              // a level the gate refuses
      const bool crowded = k > 0 && i != 0 && j >= n - crowd;                      // one of the `crowd` features around world point 0
      if (i == 0 || crowded) oct = level[0];
      const double s = kf->mvScaleFactors[oct];
      float u = (float)(458 * xc / zc + 367 + g.normal() * s), v = (float)(457 * yc / zc + 248 + g.normal() * s);
      bool gross = g.uni() < 0.1;
      if (i == 0) { gross = false; u = (float)u0; v = (float)v0; }
      if (crowded) { gross = true; u = (float)(u0 + g.range(-1.5, 1.5)); v = (float)(v0 + g.range(-1.5, 1.5)); }
      else if (gross) { u = (float)g.range(-4, 756); v = (float)g.range(-4, 484); } // somewhere else (also off the grid)
      const mock::KeyPoint kp{{u, v}, (float)(31 * s), (float)g.range(0, 360), 0.f, oct};
      kf->mvKeysUn.push_back(kp);
      const bool stereo = !mono && g.uni() < 0.5 && !crowded && i != 0;
      kf->mvDepth.push_back(stereo ? (float)zc : -1.f);
      kf->mvuRight.push_back(stereo ? (float)(u - kf->mbf / zc + g.normal() * 0.4 * s) : -1.f);
      std::vector<uint8_t> d = base[i];
      for (int f = g.below(60); f > 0; f--) { const int bit = g.below(256); d[bit >> 3] ^= (uint8_t)(1 << (bit & 7)); }
      if (crowded) for (auto& b : d) b = (uint8_t)g.below(256);
      if (i == 0) {                                                                // the point's own descriptor with k bits flipped: the best match
        std::memcpy(d.data(), first[0]->GetDescriptor().ptr<uint8_t>(0), 32);      // by far, and another descriptor after ComputeDistinctiveDescriptors
        for (int bit = 0; bit < k; bit++) d[bit >> 3] ^= (uint8_t)(1 << (bit & 7));
      }
      std::memcpy(kf->mDescriptors.ptr<uint8_t>(j), d.data(), 32);
      const double r = g.uni();
      MapPoint* p = gross ? nullptr : (r < 0.4 ? first[i] : (r < 0.6 ? second[i] : nullptr));
      if (i == 0) p = k == 1 ? second[0] : (k == 2 ? nullptr : first[0]);          // the duplicate sits in the first target only
      if (p) { mps[j] = p; held.emplace_back(p, j); }
    }
    kf->TestSetMapPoints(mps);
    kf->TestBuildGrid();
    for (auto& h : held) h.first->AddObservation(kf.get(), h.second);
    w.kfs.push_back(std::move(kf));
  }
  // covisibility: the current keyframe names kfs[1 .. listed]; each of those names the current one and two listed ones (second
  // neighbours that repeat), and every other keyframe is named by two listed ones
  std::vector<KeyFrame*> nb;
  for (int k = 1; k <= listed; k++) nb.push_back(w.kfs[k].get());
  w.kfs[0]->TestSetNeighbours(nb);
  const int others = chain ? std::max(listed, nkf - 3) : nkf;                      // the last three come in through the mPrevKF chain only
  std::vector<std::vector<KeyFrame*>> sn(listed + 1);
  for (int k = 1; k <= listed; k++) sn[k] = {w.kfs[0].get(), w.kfs[1 + k % listed].get(), w.kfs[1 + (k + 2) % listed].get()};
  for (int q = listed + 1; q <= others; q++) { sn[1 + q % listed].push_back(w.kfs[q].get()); sn[1 + (q * 7 + 3) % listed].push_back(w.kfs[q].get()); }
  for (int k = 1; k <= listed; k++) w.kfs[k]->TestSetNeighbours(sn[k]);
  const int bad = listed + 2 <= nkf ? listed + 2 : -1;
  if (bad > 0) w.kfs[bad]->TestSetBad();
  if (chain) {                                                                     // new, already a target, new, the bad one, new
    std::vector<int> order;
    for (int q : {nkf, 1, nkf - 1, bad, nkf - 2})
      if (q >= 1 && q <= nkf && std::find(order.begin(), order.end(), q) == order.end()) order.push_back(q);
    KeyFrame* at = w.kfs[0].get();
    for (int q : order) { at->mPrevKF = w.kfs[q].get(); at = at->mPrevKF; }
  }
}

static void dump(const char* tag, const World& w) {
  std::printf("[%s]\n", tag);
  for (size_t k = 0; k < w.kfs.size(); k++) {
    const auto mps = w.kfs[k]->GetMapPointMatches();
    std::printf("kf%zu: target=%lu connections=%d points:", k, w.kfs[k]->mnFuseTargetForKF, w.kfs[k]->n_update_connections);
    for (size_t i = 0; i < mps.size(); i++) if (mps[i]) std::printf(" %zu=%lu", i, mps[i]->mnId);
    std::printf("\n");
  }
  for (const auto& p : w.points) {
    std::printf("mp%lu: bad=%d replaced=%lu nobs=%d cand=%lu distinctive=%d normal=%d desc=", p->mnId, (int)p->isBad(),
                p->TestReplaced() ? p->TestReplaced()->mnId : 0ul, p->Observations(), p->mnFuseCandidateForKF, p->n_distinctive, p->n_normal_updates);
    const auto D = p->GetDescriptor();
    for (int b = 0; b < 32; b++) std::printf("%02x", D.ptr<uint8_t>(0)[b]);
    std::printf(" obs:");
    for (const auto& ob : p->TestObservations()) std::printf(" %lu/%d", ob.first->mnId, ob.second);
    std::printf("\n");
  }
}

struct AbortAt {                  // mbAbortBA: true from its k-th reading on (0: never)
  int k, reads = 0;
  bool operator()() { reads++; return k > 0 && reads >= k; }
};

static void run_scene(const char* name, uint64_t seed, int n, int nkf, int listed, bool mono, bool inertial, int abort_after) {
  World a, b;
  build(a, seed, n, nkf, listed, mono, inertial, 24);
  build(b, seed, n, nkf, listed, mono, inertial, 24);
  AbortAt fa{abort_after}, fb{abort_after};
  orbgpu::KeyFramesOnDevice<KeyFrame> dev;
  orbgpu::FuseStats st;
  const int ra = orbgpu::SearchInNeighbors(a.kfs[0].get(), dev, mono, inertial, std::ref(fa), &st);
  const int rb = fuse_ref::SearchInNeighbors(b.kfs[0].get(), mono, inertial, std::ref(fb));
  std::printf("[%s]\ntargets: %d %d\nabort_reads: %d %d\nresident: %zu\nstats: pairs=%ld rescored=%ld relaunched=%ld\n", name, ra, rb, fa.reads, fb.reads,
              dev.size(), st.pairs, st.rescored, st.relaunched);
  char tag[64];
  std::snprintf(tag, sizeof tag, "%s.glue", name); dump(tag, a);
  std::snprintf(tag, sizeof tag, "%s.ref", name); dump(tag, b);
}

// ORBmatcher::Fuse on its own: every point of the map into one keyframe, descriptors of some points changed after the map was built
static void run_fuse(const char* name, uint64_t seed, int n) {
  World a, b;
  build(a, seed, n, 3, 3, false, false);
  build(b, seed, n, 3, 3, false, false);
  int fused[2];
  int side = 0;
  for (World* w : {&a, &b}) {
    std::vector<MapPoint*> all;
    for (auto& p : w->points) all.push_back(p.get());
    all.insert(all.begin() + 3, nullptr);
    if (side == 0) { orbgpu::KeyFramesOnDevice<KeyFrame> dev; fused[0] = orbgpu::Fuse(w->kfs[2].get(), all, 4.0f, dev); }
    else fused[1] = fuse_ref::Fuse(w->kfs[2].get(), all, 4.0f);
    side++;
  }
  std::printf("[%s]\nfused: %d %d\n", name, fused[0], fused[1]);
  char tag[64];
  std::snprintf(tag, sizeof tag, "%s.glue", name); dump(tag, a);
  std::snprintf(tag, sizeof tag, "%s.ref", name); dump(tag, b);
}

// a keyframe of a rig among the targets is out of scope: nothing is touched, no mark written
static void run_rig(uint64_t seed) {
  World c, d;
  build(c, seed, 40, 6, 3, false, false);
  build(d, seed, 40, 6, 3, false, false);
  c.kfs[4]->NLeft = 20;                                       // a second neighbour (kfs[5] is the bad keyframe: never a target)
  AbortAt f{0};
  orbgpu::KeyFramesOnDevice<KeyFrame> dev;
  const int r = orbgpu::SearchInNeighbors(c.kfs[0].get(), dev, false, false, std::ref(f));
  std::printf("[rig]\nreturned: %d\nresident: %zu\n", r, dev.size());
  dump("rig.glue", c);
  dump("rig.ref", d);                                         // the untouched map
}

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static int run_time(int n, int targets, bool mono, int reps) {
  const int listed = std::min(targets, mono ? 20 : 10);
  orbgpu::KeyFramesOnDevice<KeyFrame> dev;
  std::vector<std::unique_ptr<World>> worlds;
  std::vector<double> us_glue, us_ref;
  orbgpu::FuseStats st;
  int ra = 0, rb = 0;
  // every repetition runs on a fresh copy of the map; its keyframes are made resident before the clock starts (a running
  // LocalMapping uploaded them when they were the current keyframe) and dropped afterwards
  for (int r = 0; r < reps + 2; r++) {
    World b;
    build(b, 77, n, targets, listed, mono, false);
    AbortAt fb{0};
    const auto t0 = std::chrono::steady_clock::now();
    rb = fuse_ref::SearchInNeighbors(b.kfs[0].get(), mono, false, std::ref(fb));
    if (r >= 2) us_ref.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  for (int r = 0; r < reps + 2; r++) {
    worlds.emplace_back(new World);
    World& a = *worlds.back();
    build(a, 77, n, targets, listed, mono, false);
    for (auto& kf : a.kfs) dev.Get(kf.get());                 // resident before the clock starts (a running system uploaded them earlier)
    AbortAt fa{0};
    orbgpu::FuseStats s1;
    const auto t0 = std::chrono::steady_clock::now();
    ra = orbgpu::SearchInNeighbors(a.kfs[0].get(), dev, mono, false, std::ref(fa), &s1);
    if (r >= 2) { us_glue.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count()); st = s1; }
    for (auto& kf : a.kfs) dev.Erase(kf.get());
  }
  std::printf("glue_us: %.1f\nrestatement_us: %.1f\ntargets: %d %d\npairs: %ld\nrescored: %ld\nrelaunched: %ld\n", median(us_glue), median(us_ref), ra, rb,
              st.pairs, st.rescored, st.relaunched);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 6 && std::strcmp(argv[1], "--time") == 0) return run_time(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) != 0, std::atoi(argv[5]));
    if (argc >= 2 && std::strcmp(argv[1], "--gpu") == 0) {
      const int abort_after = argc >= 3 ? std::atoi(argv[2]) : 0;
      run_scene("stereo", 21, 180, 9, 4, false, false, abort_after);
      run_scene("mono_inertial", 22, 150, 10, 4, true, true, abort_after);
      run_fuse("fuse", 23, 120);
      run_rig(24);
      return 0;
    }
    std::fprintf(stderr, "usage: fuse_glue --gpu [abort_after] | --time n targets mono reps\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fuse_glue: %s\n", e.what());
    return 2;
  }
}
