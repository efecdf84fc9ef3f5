// orbgpu::TwoViewReconstruction (include/orbgpu_dropin.hpp) with the reference's constructor and Reconstruct signature over the mock
// Mat / KeyPoint of mock_orbslam3.hpp (-DHAVE_OPENCV: over cv::Mat / cv::KeyPoint of the signature-only stub in opencv_stub).
//   two_view_glue <scene.bin> <iterations>
// scene.bin: int32 n1, n2; float fx, fy, cx, cy; keys1 (n1 x 2 float); keys2 (n2 x 2 float); matches12 (n1 int32).
// Prints the return value, every raw draw the default functor took (RandomInt after SeedRandOnce(0)) and the outputs with their float
// bits; tests/test_two_view_glue.py hands the same draws to the Python API and compares.  Fewer than eight matches: "ok 0" without a
// device.  Exit code 3 + "no usable HIP device" without a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#ifdef HAVE_OPENCV
#include <opencv2/core/core.hpp>
#endif
#include "mock_orbslam3.hpp"
#include "orbgpu_dropin.hpp"

#ifdef HAVE_OPENCV
typedef cv::Mat MatT;
typedef cv::KeyPoint KeyPointT;
static MatT make_K(const float* k) { MatT m(3, 3, CV_32F); std::memcpy(m.ptr<float>(0), k, 36); return m; }
static KeyPointT make_kp(float x, float y) { return KeyPointT(x, y, 31.f); }
#else
typedef mock::Mat MatT;
typedef mock::KeyPoint KeyPointT;
static MatT make_K(const float* k) { MatT m(3, 3, 4); std::memcpy(m.ptr<float>(0), k, 36); return m; }
static KeyPointT make_kp(float x, float y) { return KeyPointT{{x, y}, 31.f, 0.f, 0.f, 0}; }
#endif
struct Point3f { float x = 0, y = 0, z = 0; };     // cv::Point3f's members

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void print_f(const char* key, const float* v, size_t n) {
  std::printf("%s:", key);
  for (size_t i = 0; i < n; i++) std::printf(" %08x", bits(v[i]));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: two_view_glue <scene.bin> <iterations>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t n[2]; float cam[4];
  if (std::fread(n, 4, 2, f) != 2 || std::fread(cam, 4, 4, f) != 4) return 2;
  std::vector<float> k1(2 * (size_t)n[0]), k2(2 * (size_t)n[1]);
  std::vector<int32_t> m(n[0]);
  if (std::fread(k1.data(), 4, k1.size(), f) != k1.size() || std::fread(k2.data(), 4, k2.size(), f) != k2.size() ||
      std::fread(m.data(), 4, m.size(), f) != m.size()) return 2;
  std::fclose(f);
  const int iterations = std::atoi(argv[2]);
  std::vector<KeyPointT> vKeys1, vKeys2;
  for (int i = 0; i < n[0]; i++) vKeys1.push_back(make_kp(k1[2 * i], k1[2 * i + 1]));
  for (int i = 0; i < n[1]; i++) vKeys2.push_back(make_kp(k2[2 * i], k2[2 * i + 1]));
  const std::vector<int> vMatches12(m.begin(), m.end());
  const float Kf[9] = {cam[0], 0, cam[2], 0, cam[1], cam[3], 0, 0, 1};
  MatT K = make_K(Kf);
  orbgpu::TwoViewReconstruction<MatT, KeyPointT, Point3f> tv(K, 1.0f, iterations);
  MatT R21, t21;
  std::vector<Point3f> vP3D;
  std::vector<bool> vbTriangulated;
  bool ok = false;
  try {
    ok = tv.Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated);
  } catch (const std::exception& e) {
    if (orbg_device_count() < 1) { std::printf("no usable HIP device\n"); return 3; }
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("ok %d\n", ok ? 1 : 0);
  std::printf("draws:");
  for (int32_t d : tv.last_draws()) std::printf(" %d", d);
  std::printf("\n");
  const orbi_two_view_result& r = tv.last();
  std::printf("model %d bestH %d bestF %d motions %d best_motion %d\n", r.model, r.best_iteration_H, r.best_iteration_F, r.n_motions, r.best_motion);
  print_f("scores", &r.SH, 1); print_f("scores", &r.SF, 1);
  if (ok) {
    print_f("R21", orbgpu::dropin::mat_f32(R21), 9);
    print_f("t21", orbgpu::dropin::mat_f32(t21), 3);
    std::printf("sizes %zu %zu\n", vP3D.size(), vbTriangulated.size());
    std::vector<float> flat;
    for (const Point3f& p : vP3D) { flat.push_back(p.x); flat.push_back(p.y); flat.push_back(p.z); }
    print_f("vP3D", flat.data(), flat.size());
    std::printf("vbTriangulated:");
    for (bool b : vbTriangulated) std::printf(" %d", b ? 1 : 0);
    std::printf("\n");
  } else {
    std::printf("outputs untouched %d\n", (int)(R21.empty() && t21.empty() && vP3D.empty() && vbTriangulated.empty()));
  }
  return 0;
}
