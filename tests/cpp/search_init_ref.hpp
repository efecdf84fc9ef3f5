// ORBmatcher::SearchForInitialization (S/ORBmatcher.cc:702-817) and Frame::GetFeaturesInArea (S/Frame.cc:628-697) restated serially
// over plain arrays, in the reference's statement order: the checker of tests/cpp/search_init_glue.cpp and of the CPU tests (which
// hold it against tests/search_init_model.py).  It shares no code with the library: its own grid, its own histogram, its own
// ComputeThreeMaxima.  A float that does not fit an int saturates (the reference's cast is undefined there).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace sref {

constexpr int COLS = 64, ROWS = 48, HISTO = 30, TH_LOW = 50;

struct Kp { float x, y, size, angle, response; int32_t octave; };

inline int to_int(float v) {
  if (!(v > -2147483648.f)) return INT_MIN;      // (also NaN)
  if (!(v < 2147483648.f)) return INT_MAX;
  return (int)v;
}

struct Frame {
  std::vector<Kp> kps;
  std::vector<uint8_t> desc;
  float min_x = 0, max_x = 0, min_y = 0, max_y = 0, w_inv = 0, h_inv = 0;
  std::vector<int> grid[COLS][ROWS];
  void assign() {                                 // S/Frame.cc:127-144, :360-391, :699-709
    w_inv = (float)COLS / (float)(max_x - min_x);
    h_inv = (float)ROWS / (float)(max_y - min_y);
    for (auto& col : grid) for (auto& c : col) c.clear();
    for (int i = 0; i < (int)kps.size(); i++) {
      const int px = to_int(std::round((kps[i].x - min_x) * w_inv)), py = to_int(std::round((kps[i].y - min_y) * h_inv));
      if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
      grid[px][py].push_back(i);
    }
  }
  std::vector<int> features_in_area(float x, float y, float r, int minLevel, int maxLevel) const {
    std::vector<int> out;
    const int nMinCellX = std::max(0, to_int(std::floor((x - min_x - r) * w_inv)));
    if (nMinCellX >= COLS) return out;
    const int nMaxCellX = std::min(COLS - 1, to_int(std::ceil((x - min_x + r) * w_inv)));
    if (nMaxCellX < 0) return out;
    const int nMinCellY = std::max(0, to_int(std::floor((y - min_y - r) * h_inv)));
    if (nMinCellY >= ROWS) return out;
    const int nMaxCellY = std::min(ROWS - 1, to_int(std::ceil((y - min_y + r) * h_inv)));
    if (nMaxCellY < 0) return out;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
      for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
        for (int j : grid[ix][iy]) {
          const Kp& kp = kps[j];
          if (bCheckLevels) {
            if (kp.octave < minLevel) continue;
            if (maxLevel >= 0 && kp.octave > maxLevel) continue;
          }
          const float distx = kp.x - x, disty = kp.y - y;
          if (std::fabs(distx) < r && std::fabs(disty) < r) out.push_back(j);
        }
    return out;
  }
};

inline int descriptor_distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
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

struct Lists { std::vector<int32_t> start; std::vector<uint32_t> entries; };

// prev: n1 x {x, y}, in/out.  lists (may be NULL): every query's candidates as index2 | dist << 16.
inline int search_for_initialization(const Frame& F1, const Frame& F2, std::vector<float>& prev, std::vector<int>& vnMatches12, int windowSize,
                                     float mfNNratio, bool mbCheckOrientation, Lists* lists = nullptr) {
  int nmatches = 0;
  const int n1 = (int)F1.kps.size(), n2 = (int)F2.kps.size();
  vnMatches12 = std::vector<int>(n1, -1);
  std::vector<int> rotHist[HISTO];
  const float factor = 1.0f / HISTO;
  std::vector<int> vMatchedDistance(n2, INT_MAX), vnMatches21(n2, -1);
  if (lists) { lists->start.assign(n1 + 1, 0); lists->entries.clear(); }
  for (int i1 = 0; i1 < n1; i1++) {
    if (lists) lists->start[i1] = (int32_t)lists->entries.size();
    const int level1 = F1.kps[i1].octave;
    if (level1 > 0) continue;
    const std::vector<int> vIndices2 = F2.features_in_area(prev[2 * i1], prev[2 * i1 + 1], (float)windowSize, level1, level1);
    if (vIndices2.empty()) continue;
    int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
    for (int i2 : vIndices2) {
      const int dist = descriptor_distance(&F1.desc[32 * (size_t)i1], &F2.desc[32 * (size_t)i2]);
      if (lists) lists->entries.push_back((uint32_t)i2 | ((uint32_t)dist << 16));
      if (vMatchedDistance[i2] <= dist) continue;
      if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }
      else if (dist < bestDist2) bestDist2 = dist;
    }
    if (bestDist <= TH_LOW) {
      if (bestDist < (float)bestDist2 * mfNNratio) {
        if (vnMatches21[bestIdx2] >= 0) { vnMatches12[vnMatches21[bestIdx2]] = -1; nmatches--; }
        vnMatches12[i1] = bestIdx2;
        vnMatches21[bestIdx2] = i1;
        vMatchedDistance[bestIdx2] = bestDist;
        nmatches++;
        if (mbCheckOrientation) {
          float rot = F1.kps[i1].angle - F2.kps[bestIdx2].angle;
          if (rot < 0.0) rot += 360.0f;
          int bin = (int)std::round(rot * factor);
          if (bin == HISTO) bin = 0;
          rotHist[bin].push_back(i1);
        }
      }
    }
  }
  if (lists) lists->start[n1] = (int32_t)lists->entries.size();
  if (mbCheckOrientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    three_maxima(rotHist, HISTO, ind1, ind2, ind3);
    for (int i = 0; i < HISTO; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int idx1 : rotHist[i])
        if (vnMatches12[idx1] >= 0) { vnMatches12[idx1] = -1; nmatches--; }
    }
  }
  for (int i1 = 0; i1 < n1; i1++)
    if (vnMatches12[i1] >= 0) { prev[2 * i1] = F2.kps[vnMatches12[i1]].x; prev[2 * i1 + 1] = F2.kps[vnMatches12[i1]].y; }
  return nmatches;
}

// scene file of the tests: int32 n1, n2, window, check_orientation; float nn_ratio, min_x, max_x, min_y, max_y; F1 keypoints (n1 x 24
// bytes), F1 descriptors (n1 x 32), F2 keypoints, F2 descriptors, prev (n1 x 2 float)
struct Scene { Frame F1, F2; std::vector<float> prev; int window = 0; bool check = true; float nn_ratio = 0; };

inline bool read_scene(const char* path, Scene& s) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t h[4]; float g[5];
  bool ok = std::fread(h, 4, 4, f) == 4 && std::fread(g, 4, 5, f) == 5 && h[0] >= 0 && h[1] >= 0;
  if (ok) {
    s.window = h[2]; s.check = h[3] != 0; s.nn_ratio = g[0];
    Frame* F[2] = {&s.F1, &s.F2};
    for (int k = 0; k < 2 && ok; k++) {
      F[k]->min_x = g[1]; F[k]->max_x = g[2]; F[k]->min_y = g[3]; F[k]->max_y = g[4];
      F[k]->kps.resize(h[k]); F[k]->desc.resize(32 * (size_t)h[k]);
      ok = std::fread(F[k]->kps.data(), sizeof(Kp), h[k], f) == (size_t)h[k] && std::fread(F[k]->desc.data(), 32, h[k], f) == (size_t)h[k];
      F[k]->assign();
    }
    s.prev.resize(2 * (size_t)h[0]);
    ok = ok && std::fread(s.prev.data(), 4, s.prev.size(), f) == s.prev.size();
  }
  std::fclose(f);
  return ok;
}

inline void print_result(const char* tag, int nmatches, const int* m12, const float* prev, int n1) {
  std::printf("%s nmatches %d\n%s matches12:", tag, nmatches, tag);
  for (int i = 0; i < n1; i++) std::printf(" %d", m12[i]);
  std::printf("\n%s prev:", tag);
  for (int i = 0; i < 2 * n1; i++) { uint32_t u; std::memcpy(&u, &prev[i], 4); std::printf(" %08x", u); }
  std::printf("\n");
}

}  // namespace sref
