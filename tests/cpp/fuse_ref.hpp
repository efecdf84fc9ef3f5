// ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false) (S/ORBmatcher.cc:1395-1605) and LocalMapping::SearchInNeighbors
// (S/LocalMapping.cc:868-976) restated serially in plain C++ over the mocks of mock_fuse.hpp, with the reference's loop structure:
// every (keyframe, point) pair is evaluated when its turn comes, against the objects as they are then.  The checker of
// tests/cpp/fuse_glue.cpp; no device, no library call.  Arithmetic: the choices csrc/fuse.hip lists (the cv::Mat product in float in
// k order, cv::norm and Mat::dot accumulated in double, PredictScale through (float)log((double)ratio), Pinhole::project left to
// right, the chi2 product in float against the double literals).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

namespace fuse_ref {

constexpr int TH_LOW = 50;

inline int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

// KeyFrame::GetFeaturesInArea, S/KeyFrame.cc:889-940 (NLeft == -1, bRight = false)
template <class KeyFrameT>
std::vector<size_t> GetFeaturesInArea(KeyFrameT* kf, const float& x, const float& y, const float& r) {
  std::vector<size_t> vIndices;
  const int mnGridCols = 64, mnGridRows = 48;
  const int nMinCellX = std::max(0, (int)std::floor((x - kf->mnMinX - r) * kf->test_w_inv));
  if (nMinCellX >= mnGridCols) return vIndices;
  const int nMaxCellX = std::min(mnGridCols - 1, (int)std::ceil((x - kf->mnMinX + r) * kf->test_w_inv));
  if (nMaxCellX < 0) return vIndices;
  const int nMinCellY = std::max(0, (int)std::floor((y - kf->mnMinY - r) * kf->test_h_inv));
  if (nMinCellY >= mnGridRows) return vIndices;
  const int nMaxCellY = std::min(mnGridRows - 1, (int)std::ceil((y - kf->mnMinY + r) * kf->test_h_inv));
  if (nMaxCellY < 0) return vIndices;
  for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
    for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
      const std::vector<size_t>& vCell = kf->test_grid[ix][iy];
      for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
        const auto& kpUn = kf->mvKeysUn[vCell[j]];
        const float distx = kpUn.pt.x - x;
        const float disty = kpUn.pt.y - y;
        if (std::fabs(distx) < r && std::fabs(disty) < r) vIndices.push_back(vCell[j]);
      }
    }
  return vIndices;
}

template <class KeyFrameT, class MapPointT>
int Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th = 3.0f) {
  const auto Tcw = pKF->GetPose(), Owm = pKF->GetCameraCenter();
  const float* T = Tcw.template ptr<float>(0);
  const float* Ow = Owm.template ptr<float>(0);
  const float &fx = pKF->fx, &fy = pKF->fy, &cx = pKF->cx, &cy = pKF->cy, &bf = pKF->mbf;
  int nFused = 0;
  const int nMPs = (int)vpMapPoints.size();
  for (int i = 0; i < nMPs; i++) {
    MapPointT* pMP = vpMapPoints[i];
    if (!pMP) continue;
    if (pMP->isBad()) continue;
    else if (pMP->IsInKeyFrame(pKF)) continue;
    const auto p3Dwm = pMP->GetWorldPos();
    const float* p3Dw = p3Dwm.template ptr<float>(0);
    float p3Dc[3];
    for (int a = 0; a < 3; a++) {
      const float t0 = T[4 * a] * p3Dw[0] + T[4 * a + 1] * p3Dw[1] + T[4 * a + 2] * p3Dw[2];
      p3Dc[a] = t0 + T[4 * a + 3];
    }
    // Depth must be positive
    if (p3Dc[2] < 0.0f) continue;
    const float invz = 1 / p3Dc[2];
    const float x = p3Dc[0], y = p3Dc[1], z = p3Dc[2];
    const float u = fx * x / z + cx, v = fy * y / z + cy;                // pCamera->project
    // Point must be inside the image
    if (!(u >= pKF->mnMinX && u < pKF->mnMaxX && v >= pKF->mnMinY && v < pKF->mnMaxY)) continue;
    const float ur = u - bf * invz;
    const float maxDistance = pMP->GetMaxDistanceInvariance();
    const float minDistance = pMP->GetMinDistanceInvariance();
    const float PO[3] = {p3Dw[0] - Ow[0], p3Dw[1] - Ow[1], p3Dw[2] - Ow[2]};
    const float dist3D = (float)std::sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
    // Depth must be inside the scale pyramid of the image
    if (dist3D < minDistance || dist3D > maxDistance) continue;
    // Viewing angle must be less than 60 deg
    const auto Pnm = pMP->GetNormal();
    const float* Pn = Pnm.template ptr<float>(0);
    if ((double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2] < 0.5 * dist3D) continue;
    int nPredictedLevel;
    {                                                                    // pMP->PredictScale(dist3D, pKF), S/MapPoint.cc:629-644
      const float ratio = pMP->TestMaxDistance() / dist3D;
      const float lg = (float)std::log((double)ratio);
      nPredictedLevel = (int)std::ceil(lg / pKF->mfLogScaleFactor);
      if (nPredictedLevel < 0) nPredictedLevel = 0;
      else if (nPredictedLevel >= pKF->mnScaleLevels) nPredictedLevel = pKF->mnScaleLevels - 1;
    }
    // Search in a radius
    const float radius = th * pKF->mvScaleFactors[nPredictedLevel];
    const std::vector<size_t> vIndices = GetFeaturesInArea(pKF, u, v, radius);
    if (vIndices.empty()) continue;
    // Match to the most similar keypoint in the radius
    const auto dMP = pMP->GetDescriptor();
    int bestDist = 256;
    int bestIdx = -1;
    for (auto vit = vIndices.begin(), vend = vIndices.end(); vit != vend; vit++) {
      size_t idx = *vit;
      const auto& kp = pKF->mvKeysUn[idx];
      const int& kpLevel = kp.octave;
      if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
      if (pKF->mvuRight[idx] >= 0) {
        // Check reprojection error in stereo
        const float &kpx = kp.pt.x, &kpy = kp.pt.y, &kpr = pKF->mvuRight[idx];
        const float ex = u - kpx, ey = v - kpy, er = ur - kpr;
        const float e2 = ex * ex + ey * ey + er * er;
        if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 7.8) continue;
      } else {
        const float &kpx = kp.pt.x, &kpy = kp.pt.y;
        const float ex = u - kpx, ey = v - kpy;
        const float e2 = ex * ex + ey * ey;
        if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 5.99) continue;
      }
      const int dist = DescriptorDistance(dMP.template ptr<uint8_t>(0), pKF->mDescriptors.template ptr<uint8_t>((int)idx));
      if (dist < bestDist) { bestDist = dist; bestIdx = (int)idx; }
    }
    // If there is already a MapPoint replace otherwise add new measurement
    if (bestDist <= TH_LOW) {
      MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
          else pMPinKF->Replace(pMP);
        }
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
  }
  return nFused;
}

// LocalMapping::SearchInNeighbors, S/LocalMapping.cc:868-976 (every keyframe has NLeft == -1).  Returns vpTargetKFs.size().
template <class KeyFrameT, class AbortFn>
int SearchInNeighbors(KeyFrameT* mpCurrentKeyFrame, bool mbMonocular, bool mbInertial, AbortFn mbAbortBA) {
  using MapPointT = typename std::remove_pointer<decltype(mpCurrentKeyFrame->GetMapPoint(0))>::type;
  // Retrieve neighbor keyframes
  int nn = 10;
  if (mbMonocular) nn = 20;
  const std::vector<KeyFrameT*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
  std::vector<KeyFrameT*> vpTargetKFs;
  for (auto vit = vpNeighKFs.begin(), vend = vpNeighKFs.end(); vit != vend; vit++) {
    KeyFrameT* pKFi = *vit;
    if (pKFi->isBad() || pKFi->mnFuseTargetForKF == mpCurrentKeyFrame->mnId) continue;
    vpTargetKFs.push_back(pKFi);
    pKFi->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
  }
  // Add some covisible of covisible
  for (int i = 0, imax = (int)vpTargetKFs.size(); i < imax; i++) {
    const std::vector<KeyFrameT*> vpSecondNeighKFs = vpTargetKFs[i]->GetBestCovisibilityKeyFrames(20);
    for (auto vit2 = vpSecondNeighKFs.begin(), vend2 = vpSecondNeighKFs.end(); vit2 != vend2; vit2++) {
      KeyFrameT* pKFi2 = *vit2;
      if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == mpCurrentKeyFrame->mnId || pKFi2->mnId == mpCurrentKeyFrame->mnId) continue;
      vpTargetKFs.push_back(pKFi2);
      pKFi2->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
    }
    if (mbAbortBA()) break;
  }
  // Extend to temporal neighbors
  if (mbInertial) {
    KeyFrameT* pKFi = mpCurrentKeyFrame->mPrevKF;
    while (vpTargetKFs.size() < 20 && pKFi) {
      if (pKFi->isBad() || pKFi->mnFuseTargetForKF == mpCurrentKeyFrame->mnId) { pKFi = pKFi->mPrevKF; continue; }
      vpTargetKFs.push_back(pKFi);
      pKFi->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
      pKFi = pKFi->mPrevKF;
    }
  }
  // Search matches by projection from current KF in target KFs
  std::vector<MapPointT*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  for (auto vit = vpTargetKFs.begin(), vend = vpTargetKFs.end(); vit != vend; vit++) Fuse(*vit, vpMapPointMatches);
  if (mbAbortBA()) return (int)vpTargetKFs.size();
  // Search matches by projection from target KFs in current KF
  std::vector<MapPointT*> vpFuseCandidates;
  vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
  for (auto vitKF = vpTargetKFs.begin(), vendKF = vpTargetKFs.end(); vitKF != vendKF; vitKF++) {
    KeyFrameT* pKFi = *vitKF;
    std::vector<MapPointT*> vpMapPointsKFi = pKFi->GetMapPointMatches();
    for (auto vitMP = vpMapPointsKFi.begin(), vendMP = vpMapPointsKFi.end(); vitMP != vendMP; vitMP++) {
      MapPointT* pMP = *vitMP;
      if (!pMP) continue;
      if (pMP->isBad() || pMP->mnFuseCandidateForKF == mpCurrentKeyFrame->mnId) continue;
      pMP->mnFuseCandidateForKF = mpCurrentKeyFrame->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }
  Fuse(mpCurrentKeyFrame, vpFuseCandidates);
  // Update points
  vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
    MapPointT* pMP = vpMapPointMatches[i];
    if (pMP) {
      if (!pMP->isBad()) {
        pMP->ComputeDistinctiveDescriptors();
        pMP->UpdateNormalAndDepth();
      }
    }
  }
  // Update connections in covisibility graph
  mpCurrentKeyFrame->UpdateConnections();
  return (int)vpTargetKFs.size();
}

}  // namespace fuse_ref
