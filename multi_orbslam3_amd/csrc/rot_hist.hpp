// Rotation-consistency vote of the ORBmatcher searches (S/ORBmatcher.cc:2312-2353), shared by the matchers (matcher.hip) and
// CreateNewMapPoints (newpoints.hip).  Host code.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace orbg {

constexpr int HISTO_LENGTH = 30;  // S/ORBmatcher.cc:38

// Rotation histogram without per-call allocations: bin counts + one reusable (bin, index) list in push order.
struct RotHist {
  int cnt[HISTO_LENGTH];
  std::vector<uint32_t>& e;
  explicit RotHist(std::vector<uint32_t>& store) : e(store) { for (int& c : cnt) c = 0; e.clear(); }
  void add(int bin, int idx) { cnt[bin]++; e.push_back(((uint32_t)bin << 24) | (uint32_t)idx); }
  // ORBmatcher::ComputeThreeMaxima, S/ORBmatcher.cc:2312-2353, on the bin sizes; calls drop(idx) for every entry outside
  template <typename DropFn>
  void reject_outside_three_maxima(DropFn drop) const {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
      const int s = cnt[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
      else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    for (const uint32_t v : e) {
      const int bin = (int)(v >> 24);
      if (bin != ind1 && bin != ind2 && bin != ind3) drop((int)(v & 0xFFFFFFu));
    }
  }
};

inline int rot_bin(float a1, float a2) {   // factor = 1/HISTO_LENGTH
  const float factor = 1.0f / HISTO_LENGTH;
  float rot = a1 - a2;
  if (rot < 0.0) rot += 360.0f;
  int bin = (int)std::round(rot * factor);
  if (bin == HISTO_LENGTH) bin = 0;
  return bin;
}

}  // namespace orbg
