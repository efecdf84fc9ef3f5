// The minimal sets of the reference's RANSAC loops (S/Sim3Solver.cc:189-206 with K = 3, S/TwoViewReconstruction.cc:81-96 with K = 8):
// vAvailableIndices starts as the identity over n entries; draw j picks position r[j] of the n - j entries left, takes the value
// there, writes the BACK entry over it and pops.  Closed form, no list: a position holds its own index unless an earlier removal wrote
// a back value over it; the later write wins where positions coincide.  At most K - 1 overwrites are ever looked through.
#pragma once

#include <hip/hip_runtime.h>

namespace orbg {

template <int K>
__host__ __device__ inline void resolve_draws(int n, const int (&r)[K], int (&idx)[K]) {
  int pos[K], val[K];              // removal j wrote val[j] (what stood at the back, position n - 1 - j) to position pos[j] = r[j]
#pragma unroll
  for (int j = 0; j < K; j++) {
    const int back = n - 1 - j;
    int v = r[j], bv = back;
#pragma unroll
    for (int i = 0; i < j; i++) {
      if (pos[i] == r[j]) v = val[i];
      if (pos[i] == back) bv = val[i];
    }
    idx[j] = v; pos[j] = r[j]; val[j] = bv;
  }
}

}  // namespace orbg
