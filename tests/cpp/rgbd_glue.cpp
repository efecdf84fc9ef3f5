// orbgpu::FrameOnDevice::RgbdCtor / RgbdCtorSubmitHost + RgbdCtorWait (include/orbgpu_adapters.hpp) on a mock Frame: the members the
// RGB-D constructor of the reference fills (S/Frame.cc:174-257), from the images Tracking::GrabImageRGBD receives.  Reads a scene file
// written by tests/test_rgbd_glue.py, runs the synchronous and the two-halves form, dumps both frames; the test holds them against
// tests/rgbd_model.py.
//   scene file: int32 w, h, channels, rgb_order, depth_type, has_dist; float32 fx, fy, cx, cy, bf, b, min_x, max_x, min_y, max_y,
//               depth_factor, k1, k2, p1, p2, k3; w*h*channels image bytes; w*h depth elements
//   dump file:  per form: int32 n; n keypoints; n keypoints (undistorted); n*32 descriptor bytes; n floats uRight; n floats depth
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "orbgpu_adapters.hpp"

namespace {
struct MockFrame {                       // the members of ORB_SLAM3::Frame the constructor writes
  int N = 0;
  std::vector<orbx_keypoint> mvKeys, mvKeysUn;
  std::vector<uint8_t> mDescriptors;
  std::vector<float> mvuRight, mvDepth;
  int Nleft = -1;
};

bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

void dump(FILE* f, const MockFrame& F) {
  const int32_t n = F.N;
  fwrite(&n, 4, 1, f);
  fwrite(F.mvKeys.data(), sizeof(orbx_keypoint), n, f);
  fwrite(F.mvKeysUn.data(), sizeof(orbx_keypoint), n, f);
  fwrite(F.mDescriptors.data(), 32, n, f);
  fwrite(F.mvuRight.data(), 4, n, f);
  fwrite(F.mvDepth.data(), 4, n, f);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: rgbd_glue scene.bin out.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hi[6];
  float hf[16];
  if (!read_all(f, hi, sizeof(hi)) || !read_all(f, hf, sizeof(hf))) { fprintf(stderr, "short scene file\n"); return 2; }
  const int w = hi[0], h = hi[1], ch = hi[2], rgb = hi[3], dtype = hi[4], has_dist = hi[5];
  const int es = dtype == ORBX_DEPTH_U16 ? 2 : 4;
  std::vector<uint8_t> img((size_t)w * h * ch), dep((size_t)w * h * es);
  if (!read_all(f, img.data(), img.size()) || !read_all(f, dep.data(), dep.size())) { fprintf(stderr, "short scene file\n"); return 2; }
  fclose(f);
  orbm_frame_view v{};
  v.fx = hf[0]; v.fy = hf[1]; v.cx = hf[2]; v.cy = hf[3]; v.bf = hf[4]; v.b = hf[5];
  v.min_x = hf[6]; v.max_x = hf[7]; v.min_y = hf[8]; v.max_y = hf[9];
  v.n_levels = 8; v.scale_factor = 1.2f;
  const float mDepthMapFactor = hf[10];
  const orbx_distortion dist{hf[11], hf[12], hf[13], hf[14], hf[15]};
  const orbx_distortion* mDistCoef = has_dist ? &dist : nullptr;
  try {
    orbgpu::ORBextractor ex(1000, 1.2f, 8, 20, 7, w, h);
    orbgpu::FrameOnDevice dev;
    const orbx_rgbd_image im = orbgpu::FrameOnDevice::RgbdImage(img.data(), ch, w * ch, rgb != 0, dep.data(), dtype, w * es, mDepthMapFactor);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    // synchronous: GrabImageRGBD's three statements and the constructor body in one call
    MockFrame A;
    A.N = dev.RgbdCtor(ex, v, mDistCoef, im, w, h, &A.mvKeys, &A.mvKeysUn, &A.mDescriptors, &A.mvuRight, &A.mvDepth);
    dump(out, A);
    // two halves: the Frame's storage is handed over once, Submit returns at once, Wait fills it
    MockFrame B;
    const int cap = 4096;
    B.mvKeys.resize(cap); B.mvKeysUn.resize(cap); B.mDescriptors.resize((size_t)cap * 32); B.mvuRight.resize(cap); B.mvDepth.resize(cap);
    ex.SetFrameOutputs(B.mvKeys.data(), B.mDescriptors.data(), B.mvuRight.data(), B.mvDepth.data(), cap);
    orbgpu::check(orbx_set_frame_outputs_un(ex.handle(), B.mvKeysUn.data()), "orbx_set_frame_outputs_un");
    {
      std::vector<uint8_t> img2 = img, dep2 = dep;
      const orbx_rgbd_image im2 = orbgpu::FrameOnDevice::RgbdImage(img2.data(), ch, w * ch, rgb != 0, dep2.data(), dtype, w * es, mDepthMapFactor);
      dev.RgbdCtorSubmitHost(ex, v, mDistCoef, im2, w, h);
    }                                       // flags == 0: the images are gone before the wait
    B.N = dev.RgbdCtorWait(ex);
    dump(out, B);
    fclose(out);
    printf("n %d %d frame_n %d\n", A.N, B.N, dev.N());
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
  return 0;
}
