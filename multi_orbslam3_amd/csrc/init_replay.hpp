// The serial half of ORBmatcher::SearchForInitialization (S/ORBmatcher.cc:729-816) over candidate lists that were gathered elsewhere:
// by init_search_kernel (search_init.hip) in the library, by a model in the tests.  Plain host C++ (no HIP header), so that a CPU
// test and a stand-alone sanitizer program run exactly what the library runs.
//
// A list entry is  index2 | dist << 16  (index2 < 65535, dist <= 256); the entries of query i1 are entries[base[i1] .. + count[i1]) in
// the order Frame::GetFeaturesInArea returns them (ix ascending, iy ascending, insertion order inside a cell).  count[i1] < 0 marks a
// feature of F1 that is no query (octave > 0, :719).  `index2` addresses angle2 / pt2 and nothing else: the library passes positions
// of its level-0 view there and translates the result afterwards.
#pragma once

#include <climits>
#include <cstdint>
#include <vector>

#include "rot_hist.hpp"

namespace orbg {

constexpr int kInitThLow = 50;      // TH_LOW, S/ORBmatcher.cc:36

struct InitReplayScratch {
  std::vector<int> matched_dist, matches21;
  std::vector<uint32_t> rot_store;
};

struct InitReplayCounters {
  int n_queries, n_candidates, n_evictions, n_rot_rejected;
};

// -> nmatches.  matches12 (n1) is written in full, prev_matched (n1 x {x, y}) only for the surviving matches (:812-814).
inline int init_search_replay(int n1, int n2, const int32_t* base, const int32_t* count, const uint32_t* entries, const float* angle1,
                              const float* angle2, const float* pt2, float nn_ratio, bool check_orientation, float* prev_matched,
                              int32_t* matches12, InitReplayScratch& S, InitReplayCounters* C) {
  int nmatches = 0;
  InitReplayCounters c = {0, 0, 0, 0};
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  S.matched_dist.assign((size_t)n2, INT_MAX);
  S.matches21.assign((size_t)n2, -1);
  RotHist rot(S.rot_store);
  for (int i1 = 0; i1 < n1; i1++) {
    if (count[i1] < 0) continue;
    c.n_queries++;
    c.n_candidates += count[i1];
    int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
    const uint32_t* e = entries + base[i1];
    for (int k = 0; k < count[i1]; k++) {
      const int i2 = (int)(e[k] & 0xFFFFu), dist = (int)(e[k] >> 16);
      if (S.matched_dist[i2] <= dist) continue;                                   // :741, before the bookkeeping
      if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }
      else if (dist < bestDist2) bestDist2 = dist;
    }
    if (bestDist > kInitThLow) continue;
    if (!((float)bestDist < (float)bestDist2 * nn_ratio)) continue;               // :758, a float32 product; bestDist2 may be INT_MAX
    if (S.matches21[bestIdx2] >= 0) {
      matches12[S.matches21[bestIdx2]] = -1;
      nmatches--;
      c.n_evictions++;
    }
    matches12[i1] = bestIdx2;
    S.matches21[bestIdx2] = i1;
    S.matched_dist[bestIdx2] = bestDist;
    nmatches++;
    if (check_orientation) rot.add(rot_bin(angle1[i1], angle2[bestIdx2]), i1);    // an evicted i1 stays in its bin
  }
  if (check_orientation)
    rot.reject_outside_three_maxima([&](int idx1) {
      if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; c.n_rot_rejected++; }
    });
  for (int i1 = 0; i1 < n1; i1++)
    if (matches12[i1] >= 0) {
      prev_matched[2 * i1] = pt2[2 * matches12[i1]];
      prev_matched[2 * i1 + 1] = pt2[2 * matches12[i1] + 1];
    }
  if (C) *C = c;
  return nmatches;
}

}  // namespace orbg
