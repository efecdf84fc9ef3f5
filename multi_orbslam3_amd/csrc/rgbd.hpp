// Shared by extractor.hip and matcher.hip: the device bodies of the RGB-D Frame constructor (S/Frame.cc:174-257) and of the two
// image conversions Tracking::GrabImageRGBD (S/Tracking.cc:1086-1142) runs in front of it.
//   rgbd_depth_one    Frame::ComputeStereoFromRGBD (S/Frame.cc:966-988) for one feature, with imDepth.convertTo(CV_32F, mDepthMapFactor)
//                     (S/Tracking.cc:1107-1108) applied to the ONE value it reads: convertTo is one float32 product per pixel, so
//                     converting the value that is read gives the bits of converting the image.
//   rgbd_tail_body    UndistortKeyPoints (:212) + ComputeStereoFromRGBD (:214) for the features a thread owns: the part of the
//                     constructor between the extraction and AssignFeaturesToGrid (:256).
//   rgbd_gray4        cvtColor(RGB / BGR / RGBA / BGRA -> GRAY) on packed 8-bit pixels, OpenCV's fixed-point form.
// Both are latency-bound and tiny (one value per feature, one pass over the image): they exist so that an RGB-D frame costs no
// launch gap and no host round trip more than a monocular one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbgpu.h"
#include "grid_build.hpp"

namespace orbg {

struct RgbdDepthArgs {
  const uint8_t* img;      // the RAW depth image in device memory (u16 counts or float32), rows `stride` bytes apart
  int type;                // ORBX_DEPTH_U16 / ORBX_DEPTH_F32
  int stride;              // bytes
  int width, height;
  int convert;             // GrabImageRGBD's condition: fabs(factor - 1.0f) > 1e-5 || type != CV_32F
  float factor;            // mDepthMapFactor as Tracking holds it (already inverted)
  float bf;                // mbf
  float* uright;           // mvuRight / mvDepth on the device
  float* depth;
  float* host_out;         // the same in mapped pinned memory, [mvuRight (n) | mvDepth (n)], may be NULL
};

// d = imDepth.at<float>(v, u) with the DISTORTED keypoint's coordinates truncated to int (float arguments of int parameters);
// d > 0: mvDepth = d, mvuRight = mvKeysUn.x - mbf / d (float32); otherwise both -1.  NaN and d <= 0 fail the test, +inf passes.
// The reference reads outside the image when the truncated coordinates leave it (undefined behaviour: cv::Mat::at checks nothing
// in a release build); here such a feature reads no memory and gets -1.  The extractor's keypoints are always inside.
__device__ __forceinline__ void rgbd_depth_one(const RgbdDepthArgs& a, float u, float v, float xu, float* ur, float* dp) {
  *ur = -1.0f; *dp = -1.0f;
  if (!(u > -1.0f && v > -1.0f && u < (float)a.width && v < (float)a.height)) return;      // (NaN coordinates fail too)
  const int col = (int)u, row = (int)v;
  const uint8_t* p = a.img + (size_t)row * (size_t)a.stride;
  float d;
  if (a.type == ORBX_DEPTH_U16) d = (float)reinterpret_cast<const uint16_t*>(p)[col];
  else d = reinterpret_cast<const float*>(p)[col];
  if (a.convert) d = d * a.factor;
  if (d > 0.0f) { *dp = d; *ur = xu - a.bf / d; }
}

// features tid, tid + nt, ... of the frame: undistortion (ua.on) as undistort_grid_kernel does it, then the depth association.
// A thread undistorts exactly the records grid_build_body<nt> makes it read afterwards.
__device__ __forceinline__ void rgbd_tail_body(const orbx_keypoint* __restrict__ kps, const UndistortArgs& ua, const RgbdDepthArgs& rd,
                                               int n, int tid, int nt) {
  for (int i = tid; i < n; i += nt) {
    orbx_keypoint k = kps[i];
    const float u = k.x, v = k.y;
    float xu = u;
    if (ua.on) {
      float yu;
      undistort_point(ua, u, v, &xu, &yu);
      k.x = xu; k.y = yu;
      ua.dst[i] = k;
      if (ua.dst_host) ua.dst_host[i] = k;
    }
    float ur, dp;
    rgbd_depth_one(rd, u, v, xu, &ur, &dp);
    rd.uright[i] = ur; rd.depth[i] = dp;
    if (rd.host_out) { rd.host_out[i] = ur; rd.host_out[n + i] = dp; }
  }
}

// OpenCV's 8-bit colour -> gray: (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 (R2Y = 4899, G2Y = 9617, B2Y = 1868, yuv_shift = 14);
// c0, c1, c2 are the pixel's first three bytes, rgb_order = mbRGB says whether the first is R or B.  A fourth channel is ignored.
__device__ __forceinline__ unsigned rgbd_gray_px(unsigned c0, unsigned c1, unsigned c2, int rgb_order) {
  const unsigned r = rgb_order ? c0 : c2, b = rgb_order ? c2 : c0;
  return (r * 4899u + c1 * 9617u + b * 1868u + 8192u) >> 14;
}

struct RgbdGrayArgs {
  const uint8_t* src;      // packed pixels, `channels` bytes each, rows src_stride bytes apart (HBM or the mapped staging slot)
  uint8_t* dst;            // gray, rows of `width` bytes (the extractor's packed image buffer)
  int width, height, channels, src_stride, rgb_order;
  int dwords;              // src and src_stride are multiples of 4: a thread's four pixels are read as 3 / 4 aligned dwords
};

// four pixels along x per thread: one trip to the source (over PCIe when it is the staging slot) with every read in flight at once
__device__ __forceinline__ void rgbd_gray4(const RgbdGrayArgs& a, int x0, int y) {
  if (x0 >= a.width || y >= a.height) return;
  const uint8_t* s = a.src + (size_t)y * (size_t)a.src_stride + (size_t)x0 * a.channels;
  uint8_t* d = a.dst + (size_t)y * a.width + x0;
  if (a.dwords && x0 + 4 <= a.width) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
    unsigned g[4];
    if (a.channels == 4) {
      uint32_t p[4];
#pragma unroll
      for (int q = 0; q < 4; q++) p[q] = s4[q];
#pragma unroll
      for (int q = 0; q < 4; q++) g[q] = rgbd_gray_px(p[q] & 255u, (p[q] >> 8) & 255u, (p[q] >> 16) & 255u, a.rgb_order);
    } else {
      const uint32_t w0 = s4[0], w1 = s4[1], w2 = s4[2];      // 12 bytes: c0 c1 c2 | c0 c1 c2 | c0 c1 c2 | c0 c1 c2
      g[0] = rgbd_gray_px(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, a.rgb_order);
      g[1] = rgbd_gray_px(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, a.rgb_order);
      g[2] = rgbd_gray_px((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, a.rgb_order);
      g[3] = rgbd_gray_px((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, a.rgb_order);
    }
    if ((a.width & 3) == 0) *reinterpret_cast<uint32_t*>(d) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
    else {
#pragma unroll
      for (int q = 0; q < 4; q++) d[q] = (uint8_t)g[q];
    }
    return;
  }
  for (int q = 0; q < 4 && x0 + q < a.width; q++)
    d[q] = (uint8_t)rgbd_gray_px(s[q * a.channels], s[q * a.channels + 1], s[q * a.channels + 2], a.rgb_order);
}

}  // namespace orbg
