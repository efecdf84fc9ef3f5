// LocalMapping::CreateNewMapPoints (S/LocalMapping.cc:520-865) for gfx950: ORBmatcher::SearchForTriangulation
// (S/ORBmatcher.cc:961-1202) against ALL neighbour keyframes and the triangulation of every match in ONE kernel launch, then the
// reference's serial bookkeeping across neighbours replayed on the host over the records.
//
// Why one launch is enough.  In this reference vbMatched2 is declared and never set (:1007,1063), so within one
// SearchForTriangulation call every feature idx1 of KF1 is matched independently of every other one.  The only serial coupling of the
// whole function is across neighbours: idx1 that received a point from neighbour i (AddMapPoint(pMP, idx1), S/LocalMapping.cc:852) is
// skipped for neighbours j > i (S/ORBmatcher.cc:1029-1035).  That is integer bookkeeping; the kernel evaluates every (neighbour, idx1)
// against has_mp as passed and the host drops what an earlier neighbour has claimed.
//
// Grid = (ceil(n1 / 16), B); a workgroup is 4 wavefronts = 16 groups of 16 lanes, one group per (neighbour b, feature idx1).
//   Match        the host merge-joins the two feature vectors node by node (a feature sits in exactly one node: one candidate range
//                per record).  The group's lanes stride over the candidates idx2 of the node in KF2, each applies the reference's
//                gates in its order (has_mp2, only_stereo, Hamming > TH_LOW, epipole, epipolar line | coarse) and keeps the smallest
//                key (dist << 20 | ~pos): the reference's running bestDist (`dist > bestDist` skips, equality replaces) picks the
//                smallest distance among the passing candidates and the LAST one in list order on ties.  A 4-step xor butterfly
//                over the 16 lanes gives the winner; a node of any size works (the lanes loop).
//   Triangulate  lane 0 of the group runs S/LocalMapping.cc:707-844 on the winner and writes the record.
// Buckets hold ~10 candidates, so 16 lanes per record keep four times as many lanes busy as a wavefront per record would, and four
// triangulations share a wavefront.  No atomics, every reduction is an integer min: two runs give the same bits.
//
// Arithmetic.  The reference's cv::Mat are CV_32F; what OpenCV does INSIDE a call on them is not part of the reference's source.  The
// choices made here (tests/newpoints_model.py restates the same ones); N-2 / N-3 are C-2 / C-3 of sim3.hip:
//   N-1  scalar C++ expressions are evaluated in the reference's types: float throughout, promoted to double where a double literal
//        or a double-returning call takes part (3.84 * unc, 5.991 * sigma2, 7.8 * sigma2, 1.0 / z, cos < 0.9998; dot() and norm()
//        return double, so `row.dot(x) + t` and `dot / (norm * norm)` are double expressions rounded once on assignment to float).
//        `100 * mvScaleFactors[octave]` (:1089) is int * float, i.e. a FLOAT product compared in float.
//   N-2  cv::Mat products of CV_32F (R12 = R1w R2w^T, t12, C2 = R2w Cw + t2w, the four factors of F12, Rwc xn, Rwc x3Dc + twc): cv::gemm
//        accumulates each entry in DOUBLE in k order, adds beta * C in double and rounds once to float.  A product of three matrices
//        rounds the intermediate matrix to float (it is a cv::Mat).
//   N-3  Mat::dot and cv::norm on CV_32F accumulate double products of the float entries in storage order.
//   N-4  K1.t().inv(): cv::invert on a 3 x 3 CV_32F: cofactors and determinant in double, d = 1 / det, each entry (cofactor * d)
//        rounded once to float.
//   N-5  a scaled row minus a row (xn(0) * Tcw.row(2) - Tcw.row(0), :732-735): float multiply, float subtract per entry.
//   N-6  x3D.rowRange(0, 3) / x3D.at<float>(3): the scalar 1.0 / w is formed in double, rounded to float, and the entries are
//        multiplied in float (C-4 of sim3.hip).
//   N-7  cos(2 * atan2(mb / 2, depth)) (:720,722) has float arguments, so the float overloads run: evaluated here as
//        (float)cos((double)(2 * (float)atan2((double)(mb / 2), (double)depth))) -- the correctly rounded float result up to the
//        double library's last bit.
//   N-8  cv::SVD::compute of the 4 x 4 A (:738) is float32 one-sided Jacobi in OpenCV and is NOT pinned to the bit.  Here: the
//        eigenvector of the smallest eigenvalue of A^T A in float64 (null_vector4.hpp, the answer KannalaBrandt8::Triangulate already
//        has in this library), rounded to float.  Triangulated points agree with an OpenCV build to float32 rounding, not to the bit;
//        the sign of x3D.at<float>(3) is whatever the rotations give (the point does not depend on it).
//   N-9  Pinhole::project(cv::Point3f): fx * x / z + cx in float, left to right (C-7 of sim3.hip).
// F12 depends on the keyframe pair only (the reference recomputes it per candidate, S/CameraModels/Pinhole.cpp:121-126): it is
// computed once per neighbour on the host, with R12, t12 and the epipole.  The F12 argument of SearchForTriangulation is unused in the
// reference, so LocalMapping::ComputeF12 is not needed.
// Built with -ffp-contract=off and correctly rounded float divide / sqrt, like the rest of the library.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "null_vector4.hpp"
#include "rot_hist.hpp"

using orbg::select_device;

// matcher.hip
int orbm_internal_kf_features(orbm_frame* f, const orbx_keypoint** d_kps, const uint8_t** d_desc, const float** d_uright,
                              const float** d_depth, const orbx_keypoint** h_kps, int* n, int* device, hipStream_t* stream);
int orbm_internal_order_after(orbm_frame* f, hipStream_t st);

namespace {

constexpr int TH_LOW = 50;          // S/ORBmatcher.cc:37
constexpr int kLanes = 16;          // lanes per record
constexpr int kThreads = 256;
constexpr unsigned kPosMask = 0xFFFFFu;   // list positions travel in 20 bits (a frame holds < 65535 features)

struct KfDev {                      // one keyframe side as the kernel reads it
  const orbx_keypoint* kps;         // mvKeysUn
  const uint8_t* desc;
  const float* uright;              // NULL: mvuRight = -1 throughout
  const float* depth;
  const float* keys_xy;             // mvKeys[i].pt or NULL (= mvKeysUn)
  const uint8_t* has_mp;
  int n, pad;
  float Tcw[12], Twc[12], Ow[3];
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  float sf[ORBG_MAX_LEVELS], sigma2[ORBG_MAX_LEVELS];
};

struct NbDev {                      // one neighbour of a launch
  KfDev kf;
  float F12[9];                     // K1^-T [t12]x R12 K2^-1
  float ep[2];                      // KF1's camera centre projected into KF2
  const uint32_t* cand;             // KF2's mFeatVec feature lists, flattened
};

struct NpArgs {
  KfDev k1;
  const NbDev* nb;
  const int2* range;                // per (b, idx1): [begin, end) in nb[b].cand; begin < 0: no common node
  orbm_newpoints_record* rec;
  int n1, only_stereo, coarse, far_points, match_only;
  float th_far, ratio_factor;       // ratioFactor = 1.5f * mfScaleFactor of KF1
};

__host__ __device__ inline int clamp_level(int o) { return o < 0 ? 0 : (o >= ORBG_MAX_LEVELS ? ORBG_MAX_LEVELS - 1 : o); }

__device__ __forceinline__ int popc256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {   // 4 x u64 popcount
  const unsigned long long x0 = ((unsigned long long)(a0.y ^ b0.y) << 32) | (a0.x ^ b0.x), x1 = ((unsigned long long)(a0.w ^ b0.w) << 32) | (a0.z ^ b0.z);
  const unsigned long long x2 = ((unsigned long long)(a1.y ^ b1.y) << 32) | (a1.x ^ b1.x), x3 = ((unsigned long long)(a1.w ^ b1.w) << 32) | (a1.z ^ b1.z);
  return __popcll(x0) + __popcll(x1) + __popcll(x2) + __popcll(x3);
}

// N-2 / N-3: a three-term product sum in double, k order
__host__ __device__ inline double dot3d(float a0, float a1, float a2, float b0, float b1, float b2) {
  return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}
// row i of a 3 x 4 row-major [R | t] applied to X: (float)(R.row(i).dot(X) + t(i))
__device__ __forceinline__ float row_map(const float* T, int i, const float* X) {
  return (float)(dot3d(T[4 * i], T[4 * i + 1], T[4 * i + 2], X[0], X[1], X[2]) + (double)T[4 * i + 3]);
}
__device__ __forceinline__ float norm3(const float* v) { return (float)sqrt(dot3d(v[0], v[1], v[2], v[0], v[1], v[2])); }

// KeyFrame::UnprojectStereo, S/KeyFrame.cc:947-963; false = the empty matrix
__device__ __forceinline__ bool unproject_stereo(const KfDev& K, int i, float* x3D) {
  const float z = K.depth ? K.depth[i] : -1.f;
  if (!(z > 0)) return false;
  const float u = K.keys_xy ? K.keys_xy[2 * i] : K.kps[i].x, v = K.keys_xy ? K.keys_xy[2 * i + 1] : K.kps[i].y;
  const float c[3] = {(u - K.cx) * z * K.invfx, (v - K.cy) * z * K.invfy, z};
#pragma unroll
  for (int r = 0; r < 3; r++) x3D[r] = row_map(K.Twc, r, c);
  return true;
}

// the reprojection gate of one keyframe, :774-800 / :802-825 (mbf is KF1's for both, :818); true = `continue`
__device__ __forceinline__ bool reproj_fails(const KfDev& K, float mbf, const float* x3D, float z, bool stereo, const orbx_keypoint& kp, float ur) {
  const float sigma = K.sigma2[clamp_level(kp.octave)];
  const float x = row_map(K.Tcw, 0, x3D), y = row_map(K.Tcw, 1, x3D);
  const float invz = (float)(1.0 / (double)z);
  if (!stereo) {
    const float errX = (K.fx * x / z + K.cx) - kp.x, errY = (K.fy * y / z + K.cy) - kp.y;
    return (double)(errX * errX + errY * errY) > 5.991 * (double)sigma;
  }
  const float u = K.fx * x * invz + K.cx;
  const float u_r = u - mbf * invz;
  const float v = K.fy * y * invz + K.cy;
  const float errX = u - kp.x, errY = v - kp.y, errX_r = u_r - ur;
  return (double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigma;
}

// S/LocalMapping.cc:707-844 for the pair (idx1, idx2); returns the status and fills the record's point fields
__device__ int triangulate_pair(const NpArgs& A, const KfDev& K2, int idx1, int idx2, orbm_newpoints_record& r) {
  const KfDev& K1 = A.k1;
  const orbx_keypoint kp1 = K1.kps[idx1], kp2 = K2.kps[idx2];
  const float ur1 = K1.uright ? K1.uright[idx1] : -1.f, ur2 = K2.uright ? K2.uright[idx2] : -1.f;
  const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
  const float xn1[3] = {(kp1.x - K1.cx) / K1.fx, (kp1.y - K1.cy) / K1.fy, 1.f};
  const float xn2[3] = {(kp2.x - K2.cx) / K2.fx, (kp2.y - K2.cy) / K2.fy, 1.f};
  float ray1[3], ray2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {      // Rwc = Rcw.t()
    ray1[i] = (float)dot3d(K1.Tcw[i], K1.Tcw[4 + i], K1.Tcw[8 + i], xn1[0], xn1[1], xn1[2]);
    ray2[i] = (float)dot3d(K2.Tcw[i], K2.Tcw[4 + i], K2.Tcw[8 + i], xn2[0], xn2[1], xn2[2]);
  }
  const float cosRays = (float)(dot3d(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
                                (sqrt(dot3d(ray1[0], ray1[1], ray1[2], ray1[0], ray1[1], ray1[2])) * sqrt(dot3d(ray2[0], ray2[1], ray2[2], ray2[0], ray2[1], ray2[2]))));
  r.cos_parallax = cosRays;
  float cosSt = cosRays + 1, cosSt1 = cosSt, cosSt2 = cosSt;
  if (st1) cosSt1 = (float)cos((double)(2 * (float)atan2((double)(K1.mb / 2), (double)K1.depth[idx1])));        // N-7
  else if (st2) cosSt2 = (float)cos((double)(2 * (float)atan2((double)(K2.mb / 2), (double)K2.depth[idx2])));
  cosSt = fminf(cosSt1, cosSt2);
  float x3D[3];
  if (cosRays < cosSt && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
    float Am[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {    // N-5
      Am[0][j] = xn1[0] * K1.Tcw[8 + j] - K1.Tcw[j];
      Am[1][j] = xn1[1] * K1.Tcw[8 + j] - K1.Tcw[4 + j];
      Am[2][j] = xn2[0] * K2.Tcw[8 + j] - K2.Tcw[j];
      Am[3][j] = xn2[1] * K2.Tcw[8 + j] - K2.Tcw[4 + j];
    }
    double S[4][4], v[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        double acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) acc += (double)Am[k][i] * (double)Am[k][j];
        S[i][j] = acc;
      }
    orbg::null_vector4(S, v);        // N-8
    const float w = (float)v[3];
    r.w = w;
    if (w == 0) return ORBM_NP_W_ZERO;
    const float inv = (float)(1.0 / (double)w);                 // N-6
#pragma unroll
    for (int i = 0; i < 3; i++) x3D[i] = (float)v[i] * inv;
  } else if (st1 && cosSt1 < cosSt2) {
    if (!unproject_stereo(K1, idx1, x3D)) return ORBM_NP_EMPTY;
  } else if (st2 && cosSt2 < cosSt1) {
    if (!unproject_stereo(K2, idx2, x3D)) return ORBM_NP_EMPTY;
  } else {
    return ORBM_NP_LOW_PARALLAX;
  }
  r.x3D[0] = x3D[0]; r.x3D[1] = x3D[1]; r.x3D[2] = x3D[2];
  const float z1 = row_map(K1.Tcw, 2, x3D);
  if (z1 <= 0) return ORBM_NP_Z1;
  const float z2 = row_map(K2.Tcw, 2, x3D);
  if (z2 <= 0) return ORBM_NP_Z2;
  if (reproj_fails(K1, K1.mbf, x3D, z1, st1, kp1, ur1)) return ORBM_NP_REPROJ1;
  if (reproj_fails(K2, K1.mbf, x3D, z2, st2, kp2, ur2)) return ORBM_NP_REPROJ2;
  const float n1v[3] = {x3D[0] - K1.Ow[0], x3D[1] - K1.Ow[1], x3D[2] - K1.Ow[2]};
  const float n2v[3] = {x3D[0] - K2.Ow[0], x3D[1] - K2.Ow[1], x3D[2] - K2.Ow[2]};
  const float dist1 = norm3(n1v), dist2 = norm3(n2v);
  if (dist1 == 0 || dist2 == 0) return ORBM_NP_DIST_ZERO;
  if (A.far_points && (dist1 >= A.th_far || dist2 >= A.th_far)) return ORBM_NP_FAR;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = K1.sf[clamp_level(kp1.octave)] / K2.sf[clamp_level(kp2.octave)];
  if (ratioDist * A.ratio_factor < ratioOctave || ratioDist > ratioOctave * A.ratio_factor) return ORBM_NP_SCALE;
  return ORBM_NP_ACCEPTED;
}

__global__ __launch_bounds__(kThreads) void newpoints_kernel(NpArgs A) {
  const int sub = threadIdx.x & (kLanes - 1);
  const int idx1 = blockIdx.x * (kThreads / kLanes) + (threadIdx.x / kLanes);
  const int b = blockIdx.y;
  const bool live = idx1 < A.n1;
  const NbDev& N = A.nb[b];
  int status = ORBM_NP_NO_NODE, begin = 0, end = 0;
  bool st1 = false;
  if (live) {
    const int2 rg = A.range[(size_t)b * A.n1 + idx1];
    st1 = A.k1.uright && A.k1.uright[idx1] >= 0;
    if (A.k1.has_mp[idx1]) status = ORBM_NP_HAS_POINT;                       // S/ORBmatcher.cc:1032
    else if (rg.x < 0) status = ORBM_NP_NO_NODE;
    else if (A.only_stereo && !st1) status = ORBM_NP_NOT_STEREO;             // :1039
    else { status = ORBM_NP_NO_MATCH; begin = rg.x; end = rg.y; }
  }
  unsigned best = 0xFFFFFFFFu;
  if (begin < end) {
    const orbx_keypoint kp1 = A.k1.kps[idx1];
    const uint4 a0 = *reinterpret_cast<const uint4*>(A.k1.desc + (size_t)idx1 * 32);
    const uint4 a1 = *reinterpret_cast<const uint4*>(A.k1.desc + (size_t)idx1 * 32 + 16);
    // epipolar line in the second image l = x1' F12 = [a b c], S/CameraModels/Pinhole.cpp:128-135
    const float* F = N.F12;
    const float la = kp1.x * F[0] + kp1.y * F[3] + F[6];
    const float lb = kp1.x * F[1] + kp1.y * F[4] + F[7];
    const float lc = kp1.x * F[2] + kp1.y * F[5] + F[8];
    const float den = la * la + lb * lb;
    for (int p = begin + sub; p < end; p += kLanes) {
      const int idx2 = (int)N.cand[p];
      if (N.kf.has_mp[idx2]) continue;                                        // :1063
      const bool st2 = N.kf.uright && N.kf.uright[idx2] >= 0;
      if (A.only_stereo && !st2) continue;                                    // :1068
      const uint4 b0 = *reinterpret_cast<const uint4*>(N.kf.desc + (size_t)idx2 * 32);
      const uint4 b1 = *reinterpret_cast<const uint4*>(N.kf.desc + (size_t)idx2 * 32 + 16);
      const int dist = popc256(a0, a1, b0, b1);
      if (dist > TH_LOW) continue;                                            // :1076 (`dist > bestDist` is the reduction below)
      const orbx_keypoint kp2 = N.kf.kps[idx2];
      if (!st1 && !st2) {                                                     // :1085-1093
        const float distex = N.ep[0] - kp2.x, distey = N.ep[1] - kp2.y;
        if (distex * distex + distey * distey < 100 * N.kf.sf[clamp_level(kp2.octave)]) continue;
      }
      if (!A.coarse) {                                                        // Pinhole::epipolarConstrain, :133-142
        const float num = la * kp2.x + lb * kp2.y + lc;
        if (den == 0) continue;
        const float dsqr = num * num / den;
        if (!((double)dsqr < 3.84 * (double)N.kf.sigma2[clamp_level(kp2.octave)])) continue;
      }
      const unsigned key = ((unsigned)dist << 20) | (kPosMask - (unsigned)(p - begin));   // smallest distance, last position on ties
      best = min(best, key);
    }
  }
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, m, kLanes));
  if (!live || sub != 0) return;
  orbm_newpoints_record r;
  r.idx2 = -1; r.dist = 0; r.x3D[0] = r.x3D[1] = r.x3D[2] = 0.f; r.w = 0.f; r.cos_parallax = 0.f;
  if (best != 0xFFFFFFFFu) {
    r.idx2 = (int)N.cand[begin + (int)(kPosMask - (best & kPosMask))];
    r.dist = (int)(best >> 20);
    status = A.match_only ? ORBM_NP_ACCEPTED : triangulate_pair(A, N.kf, idx1, r.idx2, r);
  }
  r.status = status;
  A.rec[(size_t)b * A.n1 + idx1] = r;
}

// ------------------------------------------------------------------------------------------------ host

// N-2: C = alpha * A * op(B), 3 x 3, double accumulation in k order, one rounding
void gemm33(const float* A, const float* Bm, bool transB, float* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      C[3 * i + j] = (float)(transB ? dot3d(A[3 * i], A[3 * i + 1], A[3 * i + 2], Bm[3 * j], Bm[3 * j + 1], Bm[3 * j + 2])
                                    : dot3d(A[3 * i], A[3 * i + 1], A[3 * i + 2], Bm[j], Bm[3 + j], Bm[6 + j]));
}
// N-4: cv::invert of a 3 x 3 CV_32F (DECOMP_LU special case); a singular matrix gives zeros as cv::invert does
void inv33(const float* S, float* T) {
  auto s = [&](int i, int j) { return (double)S[3 * i + j]; };
  double d = s(0, 0) * (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) - s(0, 1) * (s(1, 0) * s(2, 2) - s(1, 2) * s(2, 0)) +
             s(0, 2) * (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0));
  if (d == 0) { for (int i = 0; i < 9; i++) T[i] = 0.f; return; }
  d = 1. / d;
  T[0] = (float)((s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) * d);
  T[1] = (float)((s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2)) * d);
  T[2] = (float)((s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1)) * d);
  T[3] = (float)((s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2)) * d);
  T[4] = (float)((s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0)) * d);
  T[5] = (float)((s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2)) * d);
  T[6] = (float)((s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0)) * d);
  T[7] = (float)((s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1)) * d);
  T[8] = (float)((s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)) * d);
}

// What depends on the keyframe pair only: the epipole (S/ORBmatcher.cc:968-973), R12 / t12 (:987-988) and
// F12 = K1.t().inv() * t12x * R12 * K2.inv() (S/CameraModels/Pinhole.cpp:123-126).
void pair_geometry(const orbm_newpoints_kf& k1, const orbm_newpoints_kf& k2, float* F12, float* ep) {
  float R1w[9], R2w[9], t1w[3], t2w[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) { R1w[3 * i + j] = k1.Tcw[4 * i + j]; R2w[3 * i + j] = k2.Tcw[4 * i + j]; }
    t1w[i] = k1.Tcw[4 * i + 3]; t2w[i] = k2.Tcw[4 * i + 3];
  }
  float C2[3];
  for (int i = 0; i < 3; i++) C2[i] = (float)(dot3d(R2w[3 * i], R2w[3 * i + 1], R2w[3 * i + 2], k1.Ow[0], k1.Ow[1], k1.Ow[2]) + (double)t2w[i]);
  ep[0] = k2.fx * C2[0] / C2[2] + k2.cx;
  ep[1] = k2.fy * C2[1] / C2[2] + k2.cy;
  float R12[9], M[9], t12[3];
  gemm33(R1w, R2w, true, R12);
  for (int i = 0; i < 9; i++) M[i] = -R12[i];                 // -R1w * R2w.t(): alpha = -1, the same sums negated
  for (int i = 0; i < 3; i++) t12[i] = (float)(dot3d(M[3 * i], M[3 * i + 1], M[3 * i + 2], t2w[0], t2w[1], t2w[2]) + (double)t1w[i]);
  const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};   // Converter-free SkewSymmetricMatrix
  const float K1t[9] = {k1.fx, 0.f, 0.f, 0.f, k1.fy, 0.f, k1.cx, k1.cy, 1.f};
  const float K2[9] = {k2.fx, 0.f, k2.cx, 0.f, k2.fy, k2.cy, 0.f, 0.f, 1.f};
  float K1ti[9], K2i[9], P1[9], P2[9];
  inv33(K1t, K1ti);
  inv33(K2, K2i);
  gemm33(K1ti, t12x, false, P1);
  gemm33(P1, R12, false, P2);
  gemm33(P2, K2i, false, F12);
}

struct NpBufs {
  orbg::StageBlock stage;
  orbg::DevBuf<orbm_newpoints_record> d_rec;
  orbg::PinnedBuf<orbm_newpoints_record> h_rec;
  std::vector<int2> range;
  std::vector<NbDev> nb;
  std::vector<uint8_t> claimed;
  std::vector<int32_t> m12;
  std::vector<uint32_t> rot_entries;
  void release_buffers() { stage.release(); d_rec.release(); h_rec.release(); }
};

struct KfHost {                     // what the frame object says about a keyframe
  const orbx_keypoint* d_kps; const uint8_t* d_desc; const float* d_uright; const float* d_depth; const orbx_keypoint* h_kps;
  int n, device; hipStream_t stream;
};

int check_kf(const orbm_newpoints_kf* k, KfHost* h) {
  if (!k || k->struct_size != sizeof(orbm_newpoints_kf) || !k->frame) return ORBG_BAD_ARG;
  if (k->n_levels < 1 || k->n_levels > ORBG_MAX_LEVELS || !k->scale_factors || !k->level_sigma2) return ORBG_BAD_ARG;
  int rc = orbm_internal_kf_features(k->frame, &h->d_kps, &h->d_desc, &h->d_uright, &h->d_depth, &h->h_kps, &h->n, &h->device, &h->stream);
  if (rc) return rc;
  if (h->n > 0 && !k->has_mp) return ORBG_BAD_ARG;
  const orbm_featvec_view& fv = k->featvec;
  if (fv.n_nodes < 0 || (fv.n_nodes > 0 && (!fv.node_id || !fv.start || (fv.start[fv.n_nodes] > 0 && !fv.feat_idx)))) return ORBG_BAD_ARG;
  const uint32_t total = fv.n_nodes > 0 ? fv.start[fv.n_nodes] : 0;
  for (int i = 0; i < fv.n_nodes; i++)                    // the kernel walks [start[j], start[j + 1]) of the staged lists
    if (fv.start[i] > fv.start[i + 1]) return ORBG_BAD_ARG;
  for (uint32_t i = 0; i < total; i++)
    if ((int)fv.feat_idx[i] >= h->n) return ORBG_BAD_ARG;
  return ORBG_OK;
}

void fill_kf(const orbm_newpoints_kf& k, const KfHost& h, KfDev* d) {
  d->kps = h.d_kps; d->desc = h.d_desc; d->uright = h.d_uright; d->depth = h.d_depth; d->keys_xy = nullptr; d->has_mp = nullptr;
  d->n = h.n; d->pad = 0;
  memcpy(d->Tcw, k.Tcw, sizeof(d->Tcw)); memcpy(d->Twc, k.Twc, sizeof(d->Twc)); memcpy(d->Ow, k.Ow, sizeof(d->Ow));
  d->fx = k.fx; d->fy = k.fy; d->cx = k.cx; d->cy = k.cy; d->invfx = k.invfx; d->invfy = k.invfy; d->mb = k.mb; d->mbf = k.mbf;
  for (int i = 0; i < ORBG_MAX_LEVELS; i++) {
    d->sf[i] = i < k.n_levels ? k.scale_factors[i] : 0.f;
    d->sigma2[i] = i < k.n_levels ? k.level_sigma2[i] : 0.f;
  }
}

// The launch: records of all B neighbours, left in W.h_rec (B * n1).  *launched = 0: nothing had a common node (records filled here).
int run_records(orbg::WorkArea<NpBufs>& W, const orbm_newpoints_kf* kf1, const KfHost& h1, const orbm_newpoints_kf* nbs, const std::vector<KfHost>& hn,
                int B, const orbm_newpoints_params* pr, bool match_only) {
  const int n1 = h1.n;
  int rc;
  if ((rc = W.open(h1.device, "misc"))) return rc;
  const size_t nrec = (size_t)B * (size_t)n1;
  if ((rc = W.h_rec.reserve(std::max<size_t>(nrec, 1)))) return rc;
  // merge-join of the feature vectors (S/ORBmatcher.cc:1021-1168): one candidate range per (b, idx1)
  W.range.assign(nrec, int2{-1, -1});
  bool any = false;
  const orbm_featvec_view& f1 = kf1->featvec;
  for (int b = 0; b < B; b++) {
    const orbm_featvec_view& f2 = nbs[b].featvec;
    int i = 0, j = 0;
    while (i < f1.n_nodes && j < f2.n_nodes) {
      if (f1.node_id[i] == f2.node_id[j]) {
        for (uint32_t a = f1.start[i]; a < f1.start[i + 1]; a++) W.range[(size_t)b * n1 + f1.feat_idx[a]] = int2{(int)f2.start[j], (int)f2.start[j + 1]};
        any = any || f1.start[i + 1] > f1.start[i];
        i++; j++;
      } else if (f1.node_id[i] < f2.node_id[j]) {
        i = (int)(std::lower_bound(f1.node_id, f1.node_id + f1.n_nodes, f2.node_id[j]) - f1.node_id);
      } else {
        j = (int)(std::lower_bound(f2.node_id, f2.node_id + f2.n_nodes, f1.node_id[i]) - f2.node_id);
      }
    }
  }
  if (!any) {
    for (size_t k = 0; k < nrec; k++) {
      orbm_newpoints_record r{};
      r.idx2 = -1; r.status = kf1->has_mp[k % (size_t)n1] ? ORBM_NP_HAS_POINT : ORBM_NP_NO_NODE;
      W.h_rec.h[k] = r;
    }
    return ORBG_OK;
  }
  // one pinned block, one H2D copy: NbDev[B], ranges, has_mp / mvKeys of KF1, then per neighbour its lists, has_mp and mvKeys
  auto n_cand = [](const orbm_featvec_view& f) { return (size_t)(f.n_nodes > 0 ? f.start[f.n_nodes] : 0); };
  size_t payload = (size_t)B * sizeof(NbDev) + nrec * sizeof(int2) + 9 * (size_t)n1;
  for (int b = 0; b < B; b++) payload += 4 * n_cand(nbs[b].featvec) + 9 * (size_t)hn[b].n;
  orbg::StageBlock& S = W.stage;
  if ((rc = S.begin(orbg::StageLayout::bound(4 + 3 * (size_t)B, payload))) || (rc = W.d_rec.reserve(nrec))) return rc;
  NpArgs A;
  fill_kf(*kf1, h1, &A.k1);
  A.k1.has_mp = S.add(kf1->has_mp, n1, true);
  if (kf1->keys_xy) A.k1.keys_xy = S.add(kf1->keys_xy, 2 * (size_t)n1, true);
  A.range = S.add(W.range.data(), nrec, true);
  W.nb.resize(B);
  for (int b = 0; b < B; b++) {
    NbDev& N = W.nb[b];
    fill_kf(nbs[b], hn[b], &N.kf);
    N.cand = S.add(nbs[b].featvec.feat_idx, n_cand(nbs[b].featvec), true);
    N.kf.has_mp = S.add(nbs[b].has_mp, hn[b].n, true);
    if (nbs[b].keys_xy) N.kf.keys_xy = S.add(nbs[b].keys_xy, 2 * (size_t)hn[b].n, true);
    pair_geometry(*kf1, nbs[b], N.F12, N.ep);
  }
  A.nb = S.add(W.nb.data(), B, true);
  A.rec = W.d_rec.p;
  A.n1 = n1; A.only_stereo = pr->only_stereo != 0; A.coarse = pr->coarse != 0; A.far_points = pr->far_points != 0; A.match_only = match_only;
  A.th_far = pr->th_far_points; A.ratio_factor = 1.5f * kf1->scale_factor;
  // KF1's frame stream; what is pending on the neighbours' streams (an upload, a constructor) is ordered in front
  hipStream_t st = h1.stream;
  orbg::StreamDrain drain{st};
  for (int b = 0; b < B; b++)
    if ((rc = orbm_internal_order_after(nbs[b].frame, st))) return rc;
  if ((rc = S.commit(st))) return rc;
  hipLaunchKernelGGL(newpoints_kernel, dim3((n1 + kThreads / kLanes - 1) / (kThreads / kLanes), B), dim3(kThreads), 0, st, A);
  ORBG_HIP(hipGetLastError());
  ORBG_HIP(hipMemcpyAsync(W.h_rec.h, W.d_rec.p, nrec * sizeof(orbm_newpoints_record), hipMemcpyDeviceToHost, st));
  ORBG_HIP(hipStreamSynchronize(st));
  return ORBG_OK;
}

int check_call(const orbm_newpoints_kf* kf1, const orbm_newpoints_kf* nbs, int B, const orbm_newpoints_params* pr, KfHost* h1, std::vector<KfHost>* hn) {
  if (!kf1 || !pr || pr->struct_size != sizeof(orbm_newpoints_params) || B < 0 || (B > 0 && !nbs)) return ORBG_BAD_ARG;
  if (B > ORBG_NEWPOINTS_MAX_NEIGHBOURS) return ORBG_CAP_EXCEEDED;
  int rc = check_kf(kf1, h1);
  if (rc) return rc;
  hn->resize(B);
  for (int b = 0; b < B; b++) {
    if ((rc = check_kf(&nbs[b], &(*hn)[b]))) return rc;
    if ((*hn)[b].device != h1->device || nbs[b].frame == kf1->frame) return ORBG_BAD_ARG;
    if (pr->check_orientation && (*hn)[b].n > 0 && !(*hn)[b].h_kps) return ORBG_BAD_ARG;
  }
  if (pr->check_orientation && h1->n > 0 && !h1->h_kps) return ORBG_BAD_ARG;
  return ORBG_OK;
}

// vMatches12 of neighbour b after the replay: the records' matches without the features in `claimed`, then the rotation vote
// (S/ORBmatcher.cc:1143-1189) over what is left
void replay_matches(NpBufs& W, const orbm_newpoints_record* R, int n1, const KfHost& h1, const KfHost& h2, bool check_orientation, int32_t* m12) {
  orbg::RotHist rotHist(W.rot_entries);
  for (int i = 0; i < n1; i++) {
    m12[i] = (R[i].idx2 >= 0 && !W.claimed[i]) ? R[i].idx2 : -1;
    if (check_orientation && m12[i] >= 0) rotHist.add(orbg::rot_bin(h1.h_kps[i].angle, h2.h_kps[m12[i]].angle), i);
  }
  if (check_orientation) rotHist.reject_outside_three_maxima([&](int idx) { m12[idx] = -1; });
}

thread_local orbg::WorkArea<NpBufs> t_area;

}  // namespace

extern "C" int orbm_create_new_points(const orbm_newpoints_kf* kf1, const orbm_newpoints_kf* neighbours, int B, const orbm_newpoints_params* params,
                                      orbm_newpoint* out, int cap, int* n_out, orbm_newpoints_record* records, int32_t* matches) {
  KfHost h1;
  std::vector<KfHost> hn;
  if (!n_out || cap < 0 || (cap > 0 && !out)) return ORBG_BAD_ARG;
  int rc = check_call(kf1, neighbours, B, params, &h1, &hn);
  if (rc) return rc;
  *n_out = 0;
  const int n1 = h1.n;
  if (B == 0 || n1 == 0) return ORBG_OK;
  orbg::WorkArea<NpBufs>& W = t_area;
  if ((rc = run_records(W, kf1, h1, neighbours, hn, B, params, false))) return rc;
  const orbm_newpoints_record* R = W.h_rec.h;
  if (records) memcpy(records, R, (size_t)B * n1 * sizeof(orbm_newpoints_record));
  W.claimed.assign(kf1->has_mp, kf1->has_mp + n1);        // GetMapPoint(idx1) != NULL as the loop goes on
  W.m12.resize(n1);
  int count = 0;
  for (int b = 0; b < B; b++) {
    const orbm_newpoints_record* Rb = R + (size_t)b * n1;
    replay_matches(W, Rb, n1, h1, hn[b], params->check_orientation != 0, W.m12.data());
    if (matches) memcpy(matches + (size_t)b * n1, W.m12.data(), (size_t)n1 * 4);
    for (int i = 0; i < n1; i++) {                       // vMatchedPairs: ascending idx1 (S/ORBmatcher.cc:1194-1199)
      if (W.m12[i] < 0 || Rb[i].status != ORBM_NP_ACCEPTED) continue;
      if (count < cap) out[count] = orbm_newpoint{b, i, Rb[i].idx2, {Rb[i].x3D[0], Rb[i].x3D[1], Rb[i].x3D[2]}};
      count++;
      W.claimed[i] = 1;                                  // mpCurrentKeyFrame->AddMapPoint(pMP, idx1), S/LocalMapping.cc:852
    }
  }
  *n_out = count;
  return count > cap ? ORBG_CAP_EXCEEDED : ORBG_OK;
}

extern "C" int orbm_search_for_triangulation(const orbm_newpoints_kf* kf1, const orbm_newpoints_kf* kf2, const orbm_newpoints_params* params,
                                             int32_t* pairs, int cap, int* n) {
  KfHost h1;
  std::vector<KfHost> hn;
  if (!n || cap < 0 || (cap > 0 && !pairs) || !kf2) return ORBG_BAD_ARG;
  int rc = check_call(kf1, kf2, 1, params, &h1, &hn);
  if (rc) return rc;
  *n = 0;
  const int n1 = h1.n;
  if (n1 == 0) return ORBG_OK;
  orbg::WorkArea<NpBufs>& W = t_area;
  if ((rc = run_records(W, kf1, h1, kf2, hn, 1, params, true))) return rc;
  W.claimed.assign((size_t)n1, 0);                        // (has_mp of KF1 is a gate of the records themselves)
  W.m12.resize(n1);
  replay_matches(W, W.h_rec.h, n1, h1, hn[0], params->check_orientation != 0, W.m12.data());
  int count = 0;
  for (int i = 0; i < n1; i++) {
    if (W.m12[i] < 0) continue;
    if (count < cap) { pairs[2 * count] = i; pairs[2 * count + 1] = W.m12[i]; }
    count++;
  }
  *n = count;
  return count > cap ? ORBG_CAP_EXCEEDED : ORBG_OK;
}
