// orbgpu::dropin::SearchForInitialization (include/orbgpu_dropin.hpp) with the reference's signature over the mock Frames of
// mock_orbslam3.hpp, against the serial restatement of search_init_ref.hpp on the same scene file (format: search_init_ref.hpp).
//   search_init_glue --ref <scene.bin>    the restatement alone, with its candidate lists: no device needed (a CPU test holds it
//                                         against tests/search_init_model.py)
//   search_init_glue --gpu <scene.bin>    the glue and the restatement; "equal 1" when return value, vnMatches12 and vbPrevMatched
//                                         (by bit) agree.  Exit code 3 + "no usable HIP device" without a GPU.
//   search_init_glue --time <scene.bin> <reps>   median time of the restatement on one core, in microseconds
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mock_orbslam3.hpp"
#include "orbgpu_dropin.hpp"
#include "search_init_ref.hpp"

static void to_mock(const sref::Frame& s, mock::Frame& F) {
  const int n = (int)s.kps.size();
  F.N = n;
  F.mvKeysUn.resize(n); F.mvKeys.resize(n);
  for (int i = 0; i < n; i++) {
    const sref::Kp& k = s.kps[i];
    F.mvKeysUn[i] = mock::KeyPoint{{k.x, k.y}, k.size, k.angle, k.response, k.octave};
    F.mvKeys[i] = F.mvKeysUn[i];
  }
  F.mDescriptors = mock::Mat(n, 32, 1);
  if (n > 0) std::memcpy(F.mDescriptors.ptr<uint8_t>(0), s.desc.data(), 32 * (size_t)n);
  F.mvuRight.assign(n, -1.f); F.mvDepth.assign(n, -1.f);                  // a monocular Frame, S/Frame.cc:303-304
  F.mvpMapPoints.assign(n, nullptr); F.mvbOutlier.assign(n, false);
  F.mnMinX = s.min_x; F.mnMaxX = s.max_x; F.mnMinY = s.min_y; F.mnMaxY = s.max_y;
  F.fx = 458.f; F.fy = 457.f; F.cx = 320.f; F.cy = 240.f; F.mbf = 0.f; F.mb = 0.f;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: search_init_glue --ref|--gpu|--time <scene.bin> [reps]\n"); return 2; }
  sref::Scene sc;
  if (!sref::read_scene(argv[2], sc)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  const int n1 = (int)sc.F1.kps.size();
  const std::string mode = argv[1];
  if (mode == "--time") {
    const int reps = argc > 3 ? std::atoi(argv[3]) : 30;
    std::vector<double> us;
    for (int r = 0; r < reps; r++) {
      std::vector<float> prev = sc.prev; std::vector<int> m12;
      const auto t0 = std::chrono::steady_clock::now();
      sref::search_for_initialization(sc.F1, sc.F2, prev, m12, sc.window, sc.nn_ratio, sc.check);
      us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    std::printf("ref_us_median %.1f\n", us.empty() ? 0.0 : us[us.size() / 2]);
    return 0;
  }
  std::vector<float> rprev = sc.prev; std::vector<int> rm12; sref::Lists lists;
  const int rn = sref::search_for_initialization(sc.F1, sc.F2, rprev, rm12, sc.window, sc.nn_ratio, sc.check, &lists);
  sref::print_result("ref", rn, rm12.data(), rprev.data(), n1);
  if (mode == "--ref") {
    std::printf("ref list_start:");
    for (int32_t v : lists.start) std::printf(" %d", v);
    std::printf("\nref entries:");
    for (uint32_t v : lists.entries) std::printf(" %u", v);
    std::printf("\n");
    return 0;
  }
  if (orbg_device_count() < 1) { std::printf("no usable HIP device\n"); return 3; }
  mock::Frame F1, F2;
  to_mock(sc.F1, F1); to_mock(sc.F2, F2);
  std::vector<mock::Point2f> vbPrevMatched(n1);
  for (int i = 0; i < n1; i++) vbPrevMatched[i] = mock::Point2f{sc.prev[2 * i], sc.prev[2 * i + 1]};
  std::vector<int> vnMatches12;
  const int gn = orbgpu::dropin::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, sc.window, sc.nn_ratio, sc.check);
  std::vector<float> gprev(2 * (size_t)n1);
  for (int i = 0; i < n1; i++) { gprev[2 * i] = vbPrevMatched[i].x; gprev[2 * i + 1] = vbPrevMatched[i].y; }
  sref::print_result("glue", gn, vnMatches12.data(), gprev.data(), n1);
  const bool equal = gn == rn && vnMatches12 == rm12 && (n1 == 0 || std::memcmp(gprev.data(), rprev.data(), 8 * (size_t)n1) == 0);
  std::printf("equal %d\n", equal ? 1 : 0);
  orbgpu::dropin::GpuOps::release();
  return equal ? 0 : 1;
}
