// A serial plain-C++ restatement of ORBmatcher::SearchForTriangulation (S/ORBmatcher.cc:961-1202, the branch without a second camera)
// and LocalMapping::CreateNewMapPoints (S/LocalMapping.cc:520-865) on the mocks: the statement order, the running bestDist and the
// `continue`s of the reference, one neighbour after the other, with the arithmetic conventions csrc/newpoints.hip lists (N-1 .. N-9).
// Test infrastructure: the checker of include/orbgpu_localmapping.hpp (tests/cpp/new_points_glue.cpp) and the CPU figure of
// tools/newpoints_time.py.  Never linked by the product.
// Two deliberate simplifications, both in the reference's favour when timed: F12 is formed once per keyframe pair (the reference
// forms it per candidate, S/CameraModels/Pinhole.cpp:123-126), and no cv::Mat is allocated anywhere.
// cv::SVD::compute (:738) is restated as what it is in OpenCV, a one-sided Jacobi iteration in float32, so created points agree
// with the library's to float32 rounding of an ill-conditioned solve, not to the bit.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace np_ref {

constexpr int TH_LOW = 50, HISTO_LENGTH = 30;

inline double dot3d(const float* a, const float* b) { return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2]; }
inline void gemm33(const float* A, const float* B, bool transB, float* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const float col[3] = {transB ? B[3 * j] : B[j], transB ? B[3 * j + 1] : B[3 + j], transB ? B[3 * j + 2] : B[6 + j]};
      C[3 * i + j] = (float)dot3d(A + 3 * i, col);
    }
}
inline void inv33(const float* S, float* T) {
  auto s = [&](int i, int j) { return (double)S[3 * i + j]; };
  double d = s(0, 0) * (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) - s(0, 1) * (s(1, 0) * s(2, 2) - s(1, 2) * s(2, 0)) + s(0, 2) * (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0));
  if (d == 0) { for (int i = 0; i < 9; i++) T[i] = 0; return; }
  d = 1. / d;
  T[0] = (float)((s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) * d); T[1] = (float)((s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2)) * d); T[2] = (float)((s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1)) * d);
  T[3] = (float)((s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2)) * d); T[4] = (float)((s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0)) * d); T[5] = (float)((s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2)) * d);
  T[6] = (float)((s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0)) * d); T[7] = (float)((s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1)) * d); T[8] = (float)((s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)) * d);
}
inline int descriptor_distance(const uint8_t* a, const uint8_t* b) {          // S/ORBmatcher.cc:2358-2374
  const int32_t* pa = reinterpret_cast<const int32_t*>(a); const int32_t* pb = reinterpret_cast<const int32_t*>(b);
  int dist = 0;
  for (int i = 0; i < 8; i++, pa++, pb++) {
    unsigned int v = *pa ^ *pb;
    v = v - ((v >> 1) & 0x55555555);
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
    dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
  }
  return dist;
}
inline void three_maxima(const std::vector<int>* histo, int L, int& ind1, int& ind2, int& ind3) {   // S/ORBmatcher.cc:2312-2353
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = (int)histo[i].size();
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// the last row of vt of the 4 x 4 A: one-sided (Hestenes) Jacobi in float32, as cv::SVD::compute on CV_32F
inline void svd_last_vt_row(const float A[4][4], float x[4]) {
  float W[4][4], V[4][4];
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { W[i][j] = A[i][j]; V[i][j] = i == j ? 1.f : 0.f; }
  for (int sweep = 0; sweep < 30; sweep++) {
    bool changed = false;
    for (int i = 0; i < 3; i++)
      for (int j = i + 1; j < 4; j++) {
        double a = 0, b = 0, p = 0;
        for (int k = 0; k < 4; k++) { a += (double)W[k][i] * W[k][i]; b += (double)W[k][j] * W[k][j]; p += (double)W[k][i] * W[k][j]; }
        if (std::abs(p) <= FLT_EPSILON * std::sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = std::hypot(p, beta);
        double c, s;
        if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = std::sqrt(delta / gamma); c = p / (gamma * s * 2); }
        else { c = std::sqrt((gamma + beta) / (gamma * 2)); s = p / (gamma * c * 2); }
        const float cf = (float)c, sf = (float)s;
        for (int k = 0; k < 4; k++) {
          const float t0 = cf * W[k][i] + sf * W[k][j], t1 = -sf * W[k][i] + cf * W[k][j];
          W[k][i] = t0; W[k][j] = t1;
          const float v0 = cf * V[k][i] + sf * V[k][j], v1 = -sf * V[k][i] + cf * V[k][j];
          V[k][i] = v0; V[k][j] = v1;
        }
        changed = true;
      }
    if (!changed) break;
  }
  int m = 0; double best = -1;
  for (int j = 0; j < 4; j++) {
    double n = 0;
    for (int k = 0; k < 4; k++) n += (double)W[k][j] * W[k][j];
    if (best < 0 || n < best) { best = n; m = j; }
  }
  for (int k = 0; k < 4; k++) x[k] = V[k][m];
}

template <class KeyFrameT>
int SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo,
                           const bool bCoarse, const bool mbCheckOrientation) {
  const auto& vFeatVec1 = pKF1->mFeatVec;
  const auto& vFeatVec2 = pKF2->mFeatVec;
  // Compute epipole in second image
  const auto Cwm = pKF1->GetCameraCenter(); const auto R2wm = pKF2->GetRotation(); const auto t2wm = pKF2->GetTranslation();
  const auto R1wm = pKF1->GetRotation(); const auto t1wm = pKF1->GetTranslation();
  const float* Cw = Cwm.template ptr<float>(0); const float* R2w = R2wm.template ptr<float>(0); const float* t2w = t2wm.template ptr<float>(0);
  const float* R1w = R1wm.template ptr<float>(0); const float* t1w = t1wm.template ptr<float>(0);
  float C2[3];
  for (int i = 0; i < 3; i++) C2[i] = (float)(dot3d(R2w + 3 * i, Cw) + (double)t2w[i]);
  const float epx = pKF2->fx * C2[0] / C2[2] + pKF2->cx, epy = pKF2->fy * C2[1] / C2[2] + pKF2->cy;
  float R12[9], M[9], t12[3];
  gemm33(R1w, R2w, true, R12);
  for (int i = 0; i < 9; i++) M[i] = -R12[i];
  for (int i = 0; i < 3; i++) t12[i] = (float)(dot3d(M + 3 * i, t2w) + (double)t1w[i]);
  // Pinhole::epipolarConstrain's F12 (S/CameraModels/Pinhole.cpp:123-126)
  const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
  const float K1t[9] = {pKF1->fx, 0.f, 0.f, 0.f, pKF1->fy, 0.f, pKF1->cx, pKF1->cy, 1.f};
  const float K2[9] = {pKF2->fx, 0.f, pKF2->cx, 0.f, pKF2->fy, pKF2->cy, 0.f, 0.f, 1.f};
  float K1ti[9], K2i[9], P1[9], P2[9], F12[9];
  inv33(K1t, K1ti); inv33(K2, K2i);
  gemm33(K1ti, t12x, false, P1); gemm33(P1, R12, false, P2); gemm33(P2, K2i, false, F12);

  int nmatches = 0;
  std::vector<int> vMatches12(pKF1->N, -1);
  std::vector<int> rotHist[HISTO_LENGTH];
  const float factor = 1.0f / HISTO_LENGTH;
  auto f1it = vFeatVec1.begin(), f1end = vFeatVec1.end();
  auto f2it = vFeatVec2.begin(), f2end = vFeatVec2.end();
  while (f1it != f1end && f2it != f2end) {
    if (f1it->first == f2it->first) {
      for (size_t i1 = 0, iend1 = f1it->second.size(); i1 < iend1; i1++) {
        const size_t idx1 = f1it->second[i1];
        if (pKF1->GetMapPoint(idx1)) continue;
        const bool bStereo1 = (!pKF1->mpCamera2 && pKF1->mvuRight[idx1] >= 0);
        if (bOnlyStereo)
          if (!bStereo1) continue;
        const auto& kp1 = pKF1->mvKeysUn[idx1];
        const uint8_t* d1 = pKF1->mDescriptors.template ptr<uint8_t>((int)idx1);
        int bestDist = TH_LOW;
        int bestIdx2 = -1;
        for (size_t i2 = 0, iend2 = f2it->second.size(); i2 < iend2; i2++) {
          const size_t idx2 = f2it->second[i2];
          if (pKF2->GetMapPoint(idx2)) continue;                               // (vbMatched2 is never set in this reference)
          const bool bStereo2 = (!pKF2->mpCamera2 && pKF2->mvuRight[idx2] >= 0);
          if (bOnlyStereo)
            if (!bStereo2) continue;
          const int dist = descriptor_distance(d1, pKF2->mDescriptors.template ptr<uint8_t>((int)idx2));
          if (dist > TH_LOW || dist > bestDist) continue;
          const auto& kp2 = pKF2->mvKeysUn[idx2];
          if (!bStereo1 && !bStereo2 && !pKF1->mpCamera2) {
            const float distex = epx - kp2.pt.x;
            const float distey = epy - kp2.pt.y;
            if (distex * distex + distey * distey < 100 * pKF2->mvScaleFactors[kp2.octave]) continue;
          }
          bool ok = bCoarse;
          if (!ok) {                                                           // Pinhole::epipolarConstrain, :128-142
            const float a = kp1.pt.x * F12[0] + kp1.pt.y * F12[3] + F12[6];
            const float b = kp1.pt.x * F12[1] + kp1.pt.y * F12[4] + F12[7];
            const float c = kp1.pt.x * F12[2] + kp1.pt.y * F12[5] + F12[8];
            const float num = a * kp2.pt.x + b * kp2.pt.y + c;
            const float den = a * a + b * b;
            if (den != 0) {
              const float dsqr = num * num / den;
              ok = dsqr < 3.84 * pKF2->mvLevelSigma2[kp2.octave];
            }
          }
          if (ok) { bestIdx2 = (int)idx2; bestDist = dist; }
        }
        if (bestIdx2 >= 0) {
          const auto& kp2 = pKF2->mvKeysUn[bestIdx2];
          vMatches12[idx1] = bestIdx2;
          nmatches++;
          if (mbCheckOrientation) {
            float rot = kp1.angle - kp2.angle;
            if (rot < 0.0) rot += 360.0f;
            int bin = (int)std::round(rot * factor);
            if (bin == HISTO_LENGTH) bin = 0;
            rotHist[bin].push_back((int)idx1);
          }
        }
      }
      f1it++; f2it++;
    } else if (f1it->first < f2it->first) {
      f1it = vFeatVec1.lower_bound(f2it->first);
    } else {
      f2it = vFeatVec2.lower_bound(f1it->first);
    }
  }
  if (mbCheckOrientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    three_maxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (size_t j = 0, jend = rotHist[i].size(); j < jend; j++) { vMatches12[rotHist[i][j]] = -1; nmatches--; }
    }
  }
  vMatchedPairs.clear();
  vMatchedPairs.reserve(nmatches);
  for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
    if (vMatches12[i] < 0) continue;
    vMatchedPairs.push_back(std::make_pair(i, (size_t)vMatches12[i]));
  }
  return nmatches;
}

// KeyFrame::UnprojectStereo, S/KeyFrame.cc:947-963
template <class KeyFrameT>
bool UnprojectStereo(KeyFrameT* pKF, int i, float* x3D) {
  const float z = pKF->mvDepth[i];
  if (!(z > 0)) return false;
  const float u = pKF->mvKeys[i].pt.x, v = pKF->mvKeys[i].pt.y;
  const float c[3] = {(u - pKF->cx) * z * pKF->invfx, (v - pKF->cy) * z * pKF->invfy, z};
  const auto Twcm = pKF->GetPoseInverse();
  const float* Twc = Twcm.template ptr<float>(0);
  for (int r = 0; r < 3; r++) x3D[r] = (float)(dot3d(Twc + 4 * r, c) + (double)Twc[4 * r + 3]);
  return true;
}

template <class MatT, class KeyFrameT, class CheckFn, class NewFn, class AddFn>
int CreateNewMapPoints(KeyFrameT* mpCurrentKeyFrame, bool mbMonocular, bool mbInertial, bool bCoarse, bool mbFarPoints, float mThFarPoints,
                       CheckFn CheckNewKeyFrames, NewFn NewMapPoint, AddFn AddToMap) {
  int nn = 10;
  if (mbMonocular) nn = 20;
  std::vector<KeyFrameT*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  if (mbInertial) {
    KeyFrameT* pKF = mpCurrentKeyFrame;
    int count = 0;
    while (((int)vpNeighKFs.size() <= nn) && (pKF->mPrevKF) && (count++ < nn)) {
      auto it = std::find(vpNeighKFs.begin(), vpNeighKFs.end(), pKF->mPrevKF);
      if (it == vpNeighKFs.end()) vpNeighKFs.push_back(pKF->mPrevKF);
      pKF = pKF->mPrevKF;
    }
  }
  const auto Tcw1m = mpCurrentKeyFrame->GetPose();
  const float* Tcw1 = Tcw1m.template ptr<float>(0);
  const auto Ow1m = mpCurrentKeyFrame->GetCameraCenter();
  const float* Ow1 = Ow1m.template ptr<float>(0);
  const float fx1 = mpCurrentKeyFrame->fx, fy1 = mpCurrentKeyFrame->fy, cx1 = mpCurrentKeyFrame->cx, cy1 = mpCurrentKeyFrame->cy;
  const float ratioFactor = 1.5f * mpCurrentKeyFrame->mfScaleFactor;
  int made = 0;
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    if (i > 0 && CheckNewKeyFrames()) return made;
    KeyFrameT* pKF2 = vpNeighKFs[i];
    const auto Ow2m = pKF2->GetCameraCenter();
    const float* Ow2 = Ow2m.template ptr<float>(0);
    const float vB[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
    const float baseline = (float)std::sqrt(dot3d(vB, vB));
    if (!mbMonocular) {
      if (baseline < pKF2->mb) continue;
    } else {
      const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
      const float ratioBaselineDepth = baseline / medianDepthKF2;
      if (ratioBaselineDepth < 0.01) continue;
    }
    std::vector<std::pair<size_t, size_t>> vMatchedIndices;
    SearchForTriangulation(mpCurrentKeyFrame, pKF2, vMatchedIndices, false, bCoarse, false);
    const auto Tcw2m = pKF2->GetPose();
    const float* Tcw2 = Tcw2m.template ptr<float>(0);
    const float fx2 = pKF2->fx, fy2 = pKF2->fy, cx2 = pKF2->cx, cy2 = pKF2->cy;
    const int nmatches = (int)vMatchedIndices.size();
    for (int ikp = 0; ikp < nmatches; ikp++) {
      const int idx1 = (int)vMatchedIndices[ikp].first, idx2 = (int)vMatchedIndices[ikp].second;
      const auto& kp1 = mpCurrentKeyFrame->mvKeysUn[idx1];
      const float kp1_ur = mpCurrentKeyFrame->mvuRight[idx1];
      const bool bStereo1 = (!mpCurrentKeyFrame->mpCamera2 && kp1_ur >= 0);
      const auto& kp2 = pKF2->mvKeysUn[idx2];
      const float kp2_ur = pKF2->mvuRight[idx2];
      const bool bStereo2 = (!pKF2->mpCamera2 && kp2_ur >= 0);
      // Check parallax between rays
      const float xn1[3] = {(kp1.pt.x - cx1) / fx1, (kp1.pt.y - cy1) / fy1, 1.f};
      const float xn2[3] = {(kp2.pt.x - cx2) / fx2, (kp2.pt.y - cy2) / fy2, 1.f};
      float ray1[3], ray2[3];
      for (int r = 0; r < 3; r++) {
        const float c1[3] = {Tcw1[r], Tcw1[4 + r], Tcw1[8 + r]}, c2[3] = {Tcw2[r], Tcw2[4 + r], Tcw2[8 + r]};
        ray1[r] = (float)dot3d(c1, xn1); ray2[r] = (float)dot3d(c2, xn2);
      }
      const float cosParallaxRays = (float)(dot3d(ray1, ray2) / (std::sqrt(dot3d(ray1, ray1)) * std::sqrt(dot3d(ray2, ray2))));
      float cosParallaxStereo = cosParallaxRays + 1;
      float cosParallaxStereo1 = cosParallaxStereo;
      float cosParallaxStereo2 = cosParallaxStereo;
      if (bStereo1) cosParallaxStereo1 = std::cos(2 * std::atan2(mpCurrentKeyFrame->mb / 2, mpCurrentKeyFrame->mvDepth[idx1]));
      else if (bStereo2) cosParallaxStereo2 = std::cos(2 * std::atan2(pKF2->mb / 2, pKF2->mvDepth[idx2]));
      cosParallaxStereo = std::min(cosParallaxStereo1, cosParallaxStereo2);
      float x3D[3];
      if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        float A[4][4];
        for (int j = 0; j < 4; j++) {
          A[0][j] = xn1[0] * Tcw1[8 + j] - Tcw1[j];
          A[1][j] = xn1[1] * Tcw1[8 + j] - Tcw1[4 + j];
          A[2][j] = xn2[0] * Tcw2[8 + j] - Tcw2[j];
          A[3][j] = xn2[1] * Tcw2[8 + j] - Tcw2[4 + j];
        }
        float v[4];
        svd_last_vt_row(A, v);
        if (v[3] == 0) continue;
        const float inv = (float)(1.0 / (double)v[3]);
        for (int r = 0; r < 3; r++) x3D[r] = v[r] * inv;
      } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        if (!UnprojectStereo(mpCurrentKeyFrame, idx1, x3D)) continue;
      } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        if (!UnprojectStereo(pKF2, idx2, x3D)) continue;
      } else {
        continue;   // No stereo and very low parallax
      }
      // Check triangulation in front of cameras
      const float z1 = (float)(dot3d(Tcw1 + 8, x3D) + (double)Tcw1[11]);
      if (z1 <= 0) continue;
      const float z2 = (float)(dot3d(Tcw2 + 8, x3D) + (double)Tcw2[11]);
      if (z2 <= 0) continue;
      // Check reprojection error in first keyframe
      const float sigmaSquare1 = mpCurrentKeyFrame->mvLevelSigma2[kp1.octave];
      const float x1 = (float)(dot3d(Tcw1, x3D) + (double)Tcw1[3]);
      const float y1 = (float)(dot3d(Tcw1 + 4, x3D) + (double)Tcw1[7]);
      const float invz1 = 1.0 / z1;
      if (!bStereo1) {
        const float errX1 = (fx1 * x1 / z1 + cx1) - kp1.pt.x, errY1 = (fy1 * y1 / z1 + cy1) - kp1.pt.y;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) continue;
      } else {
        const float u1 = fx1 * x1 * invz1 + cx1;
        const float u1_r = u1 - mpCurrentKeyFrame->mbf * invz1;
        const float v1 = fy1 * y1 * invz1 + cy1;
        const float errX1 = u1 - kp1.pt.x, errY1 = v1 - kp1.pt.y, errX1_r = u1_r - kp1_ur;
        if ((errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * sigmaSquare1) continue;
      }
      // Check reprojection error in second keyframe
      const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
      const float x2 = (float)(dot3d(Tcw2, x3D) + (double)Tcw2[3]);
      const float y2 = (float)(dot3d(Tcw2 + 4, x3D) + (double)Tcw2[7]);
      const float invz2 = 1.0 / z2;
      if (!bStereo2) {
        const float errX2 = (fx2 * x2 / z2 + cx2) - kp2.pt.x, errY2 = (fy2 * y2 / z2 + cy2) - kp2.pt.y;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) continue;
      } else {
        const float u2 = fx2 * x2 * invz2 + cx2;
        const float u2_r = u2 - mpCurrentKeyFrame->mbf * invz2;                  // (the current keyframe's mbf, :818)
        const float v2 = fy2 * y2 * invz2 + cy2;
        const float errX2 = u2 - kp2.pt.x, errY2 = v2 - kp2.pt.y, errX2_r = u2_r - kp2_ur;
        if ((errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * sigmaSquare2) continue;
      }
      // Check scale consistency
      const float n1[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]};
      const float n2[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
      const float dist1 = (float)std::sqrt(dot3d(n1, n1)), dist2 = (float)std::sqrt(dot3d(n2, n2));
      if (dist1 == 0 || dist2 == 0) continue;
      if (mbFarPoints && (dist1 >= mThFarPoints || dist2 >= mThFarPoints)) continue;
      const float ratioDist = dist2 / dist1;
      const float ratioOctave = mpCurrentKeyFrame->mvScaleFactors[kp1.octave] / pKF2->mvScaleFactors[kp2.octave];
      if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) continue;
      // Triangulation is succesfull
      MatT X(3, 1, 4);
      for (int r = 0; r < 3; r++) X.template ptr<float>(r)[0] = x3D[r];
      auto* pMP = NewMapPoint(X, mpCurrentKeyFrame);
      pMP->AddObservation(mpCurrentKeyFrame, idx1);
      pMP->AddObservation(pKF2, idx2);
      mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
      pKF2->AddMapPoint(pMP, idx2);
      pMP->ComputeDistinctiveDescriptors();
      pMP->UpdateNormalAndDepth();
      AddToMap(pMP);
      made++;
    }
  }
  return made;
}

}  // namespace np_ref
