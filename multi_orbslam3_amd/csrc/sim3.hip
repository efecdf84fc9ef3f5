// Sim3Solver (S/Sim3Solver.cc, I/Sim3Solver.h) for gfx950: every RANSAC hypothesis of a call -- and of every problem of a batch --
// is evaluated in ONE kernel launch, then the reference's serial choice among them is replayed over the inlier counts in draw order.
//
// Grid = (hypothesis groups, problems); a workgroup is 4 wavefronts and owns kGroup = 16 consecutive hypotheses of one problem.
//   Phase A  one lane per hypothesis: raw draws -> three indices, ComputeSim3 (:301-407) in the reference's types.
//   Phase B  one wavefront per hypothesis, lanes over correspondences: CheckInliers (:410-437); __ballot gives 64 mask bits per step,
//            popcount the count.  The problem's points are staged through LDS in tiles of kTile correspondences (12 floats each): a
//            problem of up to kTile pairs sits in LDS whole, a larger one passes through in chunks -- there is no cap on n or H.
//   Phase C  the workgroup of a problem that takes the last ticket scans the H counts in draw order (replay of :184-233) and writes
//            one record: converged, iteration index, count, T12 / R / t / s and the mask of the chosen hypothesis.
// Every reduction has a fixed order (ballot + popcount are integer, the scan is a max), so two runs give identical bits.
//
// Arithmetic.  The reference's cv::Mat are CV_32F; what OpenCV does INSIDE a call on them is not part of the reference's source.
// The choices made here (the checker in tests/sim3_model.py restates the same ones and is itself compared with a float64 evaluation):
//   C-1  cv::reduce(SUM) over three float columns: ((p0 + p1) + p2) in float; C / P.cols: multiplication by (float)(1.0 / 3).
//   C-2  3x3 products (Pr2 * Pr1^T, R * Pr2, R * O2, R * X + t, sRinv * t): cv::gemm on CV_32F accumulates each entry in DOUBLE, in
//        k order, applies alpha / beta in double and rounds once to float (GEMMSingleMul<float, double>).
//   C-3  Mat::dot and cv::norm on CV_32F accumulate double products of the float entries in storage order.
//   C-4  a scaled matrix (s * R, (1.0 / s) * R^t, 2 * ang / norm * vec): the scalar is formed in double, rounded to float, and the
//        entries are multiplied in float (cv::Mat::convertTo on CV_32F).
//   C-5  cv::eigen on a symmetric CV_32F matrix runs a Jacobi iteration in float.  Here: CYCLIC Jacobi, sweep order (0,1) (0,2) (0,3)
//        (1,2) (1,3) (2,3), rotation t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq); from the fifth
//        sweep on an off-diagonal entry that no longer changes either diagonal entry (|a_pp| + 100 |a_pq| == |a_pp|, same for q) is set to
//        zero; the iteration stops when the off-diagonal sum is zero (or NaN) or after kMaxSweeps sweeps.  The eigenvector of the
//        largest eigenvalue is taken (first one on a tie); its sign is whatever the rotations give -- R does not depend on it.
//   C-6  cv::Rodrigues computes in double from the float vector and rounds R to float: theta = sqrt(x^2 + y^2 + z^2), R = I when
//        theta < DBL_EPSILON, else R = cos * I + (1 - cos) * r r^T + sin * [r]x with r = v / theta, summed left to right.
//   C-7  Pinhole::project(cv::Point3f) (S/CameraModels/Pinhole.cpp:41-52 evaluated in float): fx * x / z + cx, left to right.
// Built with -ffp-contract=off and correctly rounded float divide / sqrt, like the rest of the library.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "resolve_draws.hpp"

using orbg::select_device;

namespace {

constexpr int kGroup = 16;       // hypotheses per workgroup
constexpr int kThreads = 256;    // 4 wavefronts, 4 hypotheses each in phase B
constexpr int kTile = 1024;      // correspondences staged in LDS at a time: 12 * 4 * 1024 = 48 KiB
constexpr int kMaxSweeps = 30;
constexpr int kHypFloats = 32;   // per hypothesis in global memory: T12[16] R[9] t[3] s, 3 unused

struct Sim3Desc {                // one problem of a launch
  int n, H, fix_scale, min_inliers, best_in, n_groups, words;   // words: 64-bit mask words per hypothesis = ceil(n / 64)
  int pad;
  long long off_pts;             // floats: X3Dc1 (3n) then X3Dc2 (3n)
  long long off_thr;             // uint32: max_err1 (n) then max_err2 (n)
  long long off_draws;           // int: 3 per hypothesis
  long long off_hyp;             // hypotheses before this problem's
  long long off_mask;            // 64-bit words before this problem's
  long long off_rmask;           // 64-bit words before this problem's record mask
  float k1[4], k2[4];            // fx fy cx cy of pKF1->mpCamera / pKF2->mpCamera
};

struct Sim3Rec {                 // what the host reads back per problem
  int converged, index, count, pad;
  float hyp[kHypFloats];
};

// vAvailableIndices = mvAllIndices (the identity) with swap-with-back removal, :191-206, for raw draws r0 in [0, n), r1 in [0, n-1),
// r2 in [0, n-2): the closed form of resolve_draws.hpp with three draws.
__host__ __device__ inline void sim3_resolve_draws(int n, int r0, int r1, int r2, int* idx) {
  const int r[3] = {r0, r1, r2};
  int o[3];
  orbg::resolve_draws<3>(n, r, o);
  idx[0] = o[0]; idx[1] = o[1]; idx[2] = o[2];
}

// C-2: one row of a 3x3 product, double accumulation in k order
__device__ __forceinline__ double dot3d(float a0, float a1, float a2, float b0, float b1, float b2) {
  return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// C-5: Jacobi rotation of the symmetric 4x4 `a` (full storage) in the (P, Q) plane, accumulated into the eigenvector columns of v
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(float (&a)[4][4], float (&v)[4][4], int sweep) {
  const float apq = a[P][Q];
  if (apq == 0.0f) return;
  const float g = 100.0f * fabsf(apq);
  if (sweep > 3 && fabsf(a[P][P]) + g == fabsf(a[P][P]) && fabsf(a[Q][Q]) + g == fabsf(a[Q][Q])) {
    a[P][Q] = 0.0f; a[Q][P] = 0.0f;
    return;
  }
  const float theta = (a[Q][Q] - a[P][P]) / (2.0f * apq);
  float t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
  if (theta < 0.0f) t = -t;
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c, h = t * apq;
  a[P][P] -= h; a[Q][Q] += h;
  a[P][Q] = 0.0f; a[Q][P] = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (r != P && r != Q) {
      const float arp = a[r][P], arq = a[r][Q];
      const float np = c * arp - s * arq, nq = s * arp + c * arq;
      a[r][P] = np; a[P][r] = np; a[r][Q] = nq; a[Q][r] = nq;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float vrp = v[r][P], vrq = v[r][Q];
    v[r][P] = c * vrp - s * vrq; v[r][Q] = s * vrp + c * vrq;
  }
}

// ComputeSim3, S/Sim3Solver.cc:301-407.  P1 / P2: the three points of the minimal set (columns of P3Dc1i / P3Dc2i), [point][xyz].
// out: T12[16] R[9] t[3] s; T12 / T21 as 3x4 for CheckInliers.
__device__ void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, float* out, float* T12, float* T21) {
  // Step 1 (:312-320, ComputeCentroid :294-299): centroids and relative coordinates (C-1)
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];   // Pr[point][xyz]
  const float third = (float)(1.0 / 3.0);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    O1[c] = ((P1[0][c] + P1[1][c]) + P1[2][c]) * third;
    O2[c] = ((P2[0][c] + P2[1][c]) + P2[2][c]) * third;
#pragma unroll
    for (int p = 0; p < 3; p++) { Pr1[p][c] = P1[p][c] - O1[c]; Pr2[p][c] = P2[p][c] - O2[c]; }
  }
  // Step 2 (:324): M = Pr2 * Pr1^T, M[i][j] = sum over points of Pr2[.][i] * Pr1[.][j] (C-2)
  float M[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[i][j] = (float)dot3d(Pr2[0][i], Pr2[1][i], Pr2[2][i], Pr1[0][j], Pr1[1][j], Pr1[2][j]);
  // Step 3 (:328-346): N11..N44 are double sums of the float entries, stored as float
  const double N11 = (double)M[0][0] + M[1][1] + M[2][2], N12 = (double)M[1][2] - M[2][1], N13 = (double)M[2][0] - M[0][2],
               N14 = (double)M[0][1] - M[1][0], N22 = (double)M[0][0] - M[1][1] - M[2][2], N23 = (double)M[0][1] + M[1][0],
               N24 = (double)M[2][0] + M[0][2], N33 = -(double)M[0][0] + M[1][1] - M[2][2], N34 = (double)M[1][2] + M[2][1],
               N44 = -(double)M[0][0] - M[1][1] + M[2][2];
  float a[4][4] = {{(float)N11, (float)N12, (float)N13, (float)N14}, {(float)N12, (float)N22, (float)N23, (float)N24},
                   {(float)N13, (float)N23, (float)N33, (float)N34}, {(float)N14, (float)N24, (float)N34, (float)N44}};
  // Step 4 (:351-355): eigenvector of the largest eigenvalue (C-5)
  float v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    const float off = ((((fabsf(a[0][1]) + fabsf(a[0][2])) + fabsf(a[0][3])) + fabsf(a[1][2])) + fabsf(a[1][3])) + fabsf(a[2][3]);
    if (!(off > 0.0f)) break;
    jacobi_rotate<0, 1>(a, v, sweep); jacobi_rotate<0, 2>(a, v, sweep); jacobi_rotate<0, 3>(a, v, sweep);
    jacobi_rotate<1, 2>(a, v, sweep); jacobi_rotate<1, 3>(a, v, sweep); jacobi_rotate<2, 3>(a, v, sweep);
  }
  float q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
  float best = a[0][0];
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (a[k][k] > best) { best = a[k][k]; q[0] = v[0][k]; q[1] = v[1][k]; q[2] = v[2][k]; q[3] = v[3][k]; }
  // :357-361: ang = atan2(norm(vec), evec(0,0)) in double; vec = 2 * ang * vec / norm(vec) (C-3, C-4; 0 / 0 = NaN is kept)
  const double nrm = sqrt(((double)q[1] * q[1] + (double)q[2] * q[2]) + (double)q[3] * q[3]);
  const double ang = atan2(nrm, (double)q[0]);
  const float alpha = (float)(2.0 * ang / nrm);
  const float rv[3] = {q[1] * alpha, q[2] * alpha, q[3] * alpha};
  // :365 cv::Rodrigues (C-6)
  float R[3][3];
  {
    const double x = rv[0], y = rv[1], z = rv[2];
    const double theta = sqrt((x * x + y * y) + z * z);
    if (theta < DBL_EPSILON) {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = i == j ? 1.0f : 0.0f;
    } else {
      const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
      const double r[3] = {x * it, y * it, z * it};
      const double rx[3][3] = {{0, -r[2], r[1]}, {r[2], 0, -r[0]}, {-r[1], r[0], 0}};
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = (float)((c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + s * rx[i][j]);
    }
  }
  // Step 5 (:369): P3 = R * Pr2 (C-2); Step 6 (:373-391): scale (C-3; cv::pow(P3, 2) squares in float)
  float s12 = 1.0f;
  if (!fix_scale) {
    float P3[3][3];   // [row][point]
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int p = 0; p < 3; p++) P3[i][p] = (float)dot3d(R[i][0], R[i][1], R[i][2], Pr2[p][0], Pr2[p][1], Pr2[p][2]);
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int p = 0; p < 3; p++) { nom += (double)Pr1[p][i] * (double)P3[i][p]; den += (double)(P3[i][p] * P3[i][p]); }
    s12 = (float)(nom / den);
  }
  // Step 7 (:395-396): t = O1 - s * R * O2, one gemm with alpha = -s, beta = 1 (C-2)
  float t[3];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = (float)(-(double)s12 * dot3d(R[i][0], R[i][1], R[i][2], O2[0], O2[1], O2[2]) + (double)O1[i]);
  // Step 8 (:400-417): T12 = [sR | t], T21 = [sRinv | -sRinv * t] (C-4, C-2)
  const float sinv = (float)(1.0 / (double)s12);
  float sRi[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) { T12[i * 4 + j] = s12 * R[i][j]; sRi[i][j] = sinv * R[j][i]; T21[i * 4 + j] = sRi[i][j]; }
    T12[i * 4 + 3] = t[i];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) T21[i * 4 + 3] = (float)(-1.0 * dot3d(sRi[i][0], sRi[i][1], sRi[i][2], t[0], t[1], t[2]));
#pragma unroll
  for (int k = 0; k < 12; k++) out[k] = T12[k];
  out[12] = 0.0f; out[13] = 0.0f; out[14] = 0.0f; out[15] = 1.0f;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) out[16 + i * 3 + j] = R[i][j];
    out[25 + i] = t[i];
  }
  out[28] = s12; out[29] = 0.0f; out[30] = 0.0f; out[31] = 0.0f;
}

// Sim3Solver::Project (:452-470) for one point: P3Dc = Rcw * X + tcw as one gemm (C-2), then Pinhole::project (C-7); the squared
// distance to `ref` is Mat::dot (C-3) rounded to float (:427-428)
__device__ __forceinline__ float reproj_err(const float* T, float x, float y, float z, const float* k, float ru, float rv) {
  const float px = (float)(dot3d(T[0], T[1], T[2], x, y, z) + (double)T[3]);
  const float py = (float)(dot3d(T[4], T[5], T[6], x, y, z) + (double)T[7]);
  const float pz = (float)(dot3d(T[8], T[9], T[10], x, y, z) + (double)T[11]);
  const float u = k[0] * px / pz + k[2], v = k[1] * py / pz + k[3];
  const float du = ru - u, dv = rv - v;
  return (float)((double)du * (double)du + (double)dv * (double)dv);
}

__global__ __launch_bounds__(kThreads) void sim3_ransac_kernel(const Sim3Desc* __restrict__ descs, const float* __restrict__ pts,
                                                               const uint32_t* __restrict__ thr, const int* __restrict__ draws,
                                                               float* __restrict__ hyp, int* __restrict__ counts,
                                                               unsigned long long* __restrict__ masks, unsigned* __restrict__ tickets,
                                                               Sim3Rec* __restrict__ recs, unsigned long long* __restrict__ rec_masks) {
  const int b = blockIdx.y, g = blockIdx.x;
  const Sim3Desc D = descs[b];
  if (g >= D.n_groups) return;                       // a batch's grid is as wide as its longest problem
  __shared__ float sX[12][kTile];                    // X1 xyz, X2 xyz, P1im1 uv, P2im2 uv, max_err1, max_err2
  __shared__ float sT[kGroup][24];                   // T12, T21 as 3x4
  __shared__ int sFlag[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = D.n, H = D.H;
  const float* X1 = pts + D.off_pts;
  const float* X2 = X1 + 3 * (size_t)n;
  const uint32_t* E1 = thr + D.off_thr;
  const uint32_t* E2 = E1 + n;

  // ---- phase A
  if (tid < kGroup) {
    const int h = g * kGroup + tid;
    if (h < H) {
      const int* dr = draws + D.off_draws + 3 * (size_t)h;
      int idx[3];
      sim3_resolve_draws(n, dr[0], dr[1], dr[2], idx);
      float P1[3][3], P2[3][3];
#pragma unroll
      for (int p = 0; p < 3; p++)
#pragma unroll
        for (int c = 0; c < 3; c++) { P1[p][c] = X1[3 * (size_t)idx[p] + c]; P2[p][c] = X2[3 * (size_t)idx[p] + c]; }
      compute_sim3(P1, P2, D.fix_scale != 0, hyp + (D.off_hyp + h) * kHypFloats, &sT[tid][0], &sT[tid][12]);
    }
  }

  // ---- phase B
  int cnt[kGroup / 4] = {0, 0, 0, 0};
  for (int t0 = 0; t0 < n; t0 += kTile) {
    const int tn = min(kTile, n - t0);
    __syncthreads();                                 // phase A's sT / the previous tile's readers
    for (int i = tid; i < tn; i += kThreads) {
      const size_t k = (size_t)(t0 + i);
      const float x1 = X1[3 * k], y1 = X1[3 * k + 1], z1 = X1[3 * k + 2], x2 = X2[3 * k], y2 = X2[3 * k + 1], z2 = X2[3 * k + 2];
      sX[0][i] = x1; sX[1][i] = y1; sX[2][i] = z1; sX[3][i] = x2; sX[4][i] = y2; sX[5][i] = z2;
      // FromCameraToImage (:472-487), C-7
      sX[6][i] = D.k1[0] * x1 / z1 + D.k1[2]; sX[7][i] = D.k1[1] * y1 / z1 + D.k1[3];
      sX[8][i] = D.k2[0] * x2 / z2 + D.k2[2]; sX[9][i] = D.k2[1] * y2 / z2 + D.k2[3];
      sX[10][i] = (float)E1[k]; sX[11][i] = (float)E2[k];      // err < mvnMaxError[i]: the size_t is converted to float (:430)
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < kGroup / 4; jj++) {
      const int j = wave * (kGroup / 4) + jj, h = g * kGroup + j;
      if (h >= H) continue;                          // wave-uniform
      float T12[12], T21[12];
#pragma unroll
      for (int k = 0; k < 12; k++) { T12[k] = sT[j][k]; T21[k] = sT[j][12 + k]; }
      unsigned long long* mrow = masks + D.off_mask + (size_t)h * D.words + (t0 >> 6);
      for (int i0 = 0; i0 < tn; i0 += 64) {
        const int i = i0 + lane;
        bool ok = false;
        if (i < tn) {
          const float e1 = reproj_err(T12, sX[3][i], sX[4][i], sX[5][i], D.k1, sX[6][i], sX[7][i]);   // P2 into camera 1 vs P1im1
          const float e2 = reproj_err(T21, sX[0][i], sX[1][i], sX[2][i], D.k2, sX[8][i], sX[9][i]);   // P1 into camera 2 vs P2im2
          ok = e1 < sX[10][i] && e2 < sX[11][i];     // a NaN error compares false: outlier
        }
        const unsigned long long bal = __ballot(ok);
        cnt[jj] += __popcll(bal);
        if (lane == 0) mrow[i0 >> 6] = bal;          // one writer per word
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < kGroup / 4; jj++) {
    const int h = g * kGroup + wave * (kGroup / 4) + jj;
    if (h < H && lane == 0) counts[D.off_hyp + h] = cnt[jj];
  }

  // ---- phase C: publish, take a ticket; the workgroup that takes the problem's last one replays the serial loop.
  // The three explicit waits: (1) every wavefront drains its OWN stores before the barrier -- thread 0's release fence waits only for
  // its own wavefront's; (2) behind the release fence, before the ticket: the write-back the fence issues must have completed when the
  // ticket becomes visible, and the compiler's own wait for it is not relied on; (3) behind the acquire fence: the invalidate it issues
  // completes asynchronously, and the barrier below must not release the other wavefronts' loads before it has.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned before = __hip_atomic_fetch_add(&tickets[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = before == (unsigned)(D.n_groups - 1);
    if (last) {
      __hip_atomic_store(&tickets[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sFlag[0] = last;
  }
  __syncthreads();
  if (!sFlag[0]) return;
  if (wave == 0) {
    // :208-229 over the counts in draw order.  An iteration updates the best when count >= best so far (carried in from earlier calls);
    // it converges when it updates AND count > min_inliers.  Without convergence the best is the LAST update.
    const int* c_ = counts + D.off_hyp;
    int run = D.best_in, conv = -1, upd_last = -1;
    for (int base = 0; base < H; base += 64) {
      const int i = base + lane;
      const int c = i < H ? c_[i] : -1;
      int v = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v = max(v, o); }
      const int prev = __shfl_up(v, 1);
      const int before = lane == 0 ? run : max(run, prev);
      const bool upd = i < H && c >= before;
      const unsigned long long bc = __ballot(upd && c > D.min_inliers), bu = __ballot(upd);
      if (bc) { conv = base + __ffsll((long long)bc) - 1; break; }
      if (bu) upd_last = base + 63 - __clzll((long long)bu);
      run = max(run, __shfl(v, 63));
    }
    if (lane == 0) sFlag[1] = conv >= 0 ? conv : upd_last;
    if (lane == 0) { Sim3Rec& r = recs[b]; r.converged = conv >= 0; r.index = conv >= 0 ? conv : upd_last; r.pad = 0; }
  }
  __syncthreads();
  const int sel = sFlag[1];
  if (tid == 0) recs[b].count = sel >= 0 ? counts[D.off_hyp + sel] : 0;
  if (sel < 0) return;
  if (tid < kHypFloats) recs[b].hyp[tid] = hyp[(D.off_hyp + sel) * kHypFloats + tid];
  for (int w = tid; w < D.words; w += kThreads) rec_masks[D.off_rmask + w] = masks[D.off_mask + (size_t)sel * D.words + w];
}

// ------------------------------------------------------------------------------------------------ host side

// SetRansacParameters, S/Sim3Solver.cc:132-157, in the reference's types: float epsilon, pow / log in double, ceil, int
int ransac_iterations(int n, double probability, int min_inliers, int max_iterations) {
  const float epsilon = (float)min_inliers / n;
  int nIterations;
  if (min_inliers == n) nIterations = 1;
  else {
    const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
    // ceil() of a NaN / an infinity converted to int is INT_MIN with the x86 conversion the reference is built for: pinned here
    nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
  }
  return std::max(1, std::min(nIterations, max_iterations));
}

struct Sim3Bufs {                // device and staging buffers of one launch (a handle's, or the calling thread's for the batch form)
  orbg::DevBuf<Sim3Desc> d_desc;
  orbg::DevBuf<float> d_pts, d_hyp;
  orbg::DevBuf<uint32_t> d_thr;
  orbg::DevBuf<int> d_draws, d_counts;
  orbg::DevBuf<unsigned long long> d_masks, d_rmasks;
  orbg::DevBuf<unsigned> d_tickets;
  orbg::DevBuf<Sim3Rec> d_recs;
  size_t tickets_ready = 0;
  std::vector<Sim3Desc> h_desc;
  std::vector<float> h_pts;
  std::vector<uint32_t> h_thr;
  std::vector<int> h_draws, h_counts;
  std::vector<Sim3Rec> h_recs;
  std::vector<unsigned long long> h_rmasks, h_masks;
  std::vector<float> h_hyp;
  long long pts_resident = -1;   // >= 0: the handle's problem is on the device already
  void release_buffers() {
    d_desc.release(); d_pts.release(); d_hyp.release(); d_thr.release(); d_draws.release(); d_counts.release(); d_masks.release();
    d_rmasks.release(); d_tickets.release(); d_recs.release();
    tickets_ready = 0; pts_resident = -1;
  }
};
using Sim3Work = orbg::WorkArea<Sim3Bufs>;

struct Sim3Job {                 // one problem of a launch, host view
  const orbm_sim3_problem* p;
  int H, min_inliers, best_in;
  const int32_t* draws;
  int32_t* hyp_n_inliers; float* hyp_T12; uint64_t* hyp_masks;   // optional per-hypothesis outputs
};

int check_problem(const orbm_sim3_problem* p) {
  if (!p || p->struct_size < sizeof(orbm_sim3_problem) || p->n < 0) return ORBG_BAD_ARG;
  if (p->n > 0 && (!p->X3Dc1 || !p->X3Dc2 || !p->max_err1 || !p->max_err2)) return ORBG_BAD_ARG;
  if (p->camera_model1 != 0 || p->camera_model2 != 0) return ORBG_BAD_ARG;      // pinhole only: nothing else is approximated
  return ORBG_OK;
}

// raw RandomInt results: iteration k draws from lists of n, n - 1, n - 2 entries (:193)
int check_draws(const int32_t* draws, int H, int n) {
  if (H > 0 && (!draws || n < 3)) return ORBG_BAD_ARG;
  for (int k = 0; k < H; k++)
    for (int j = 0; j < 3; j++)
      if (draws[3 * k + j] < 0 || draws[3 * k + j] > n - 1 - j) return ORBG_BAD_ARG;
  return ORBG_OK;
}

// One launch over `jobs` (each with H >= 1, n >= 3, checked).  recs / rec masks land in w.h_recs / w.h_rmasks (job order; the mask of
// job b starts at word h_desc[b].off_rmask).  reuse_pts: job 0's points and thresholds are on the device from an earlier launch.
int launch(Sim3Work& w, const std::vector<Sim3Job>& jobs, bool reuse_pts) {
  const int B = (int)jobs.size();
  hipStream_t st = w.stream;
  w.h_desc.resize(B);
  long long o_pts = 0, o_thr = 0, o_draws = 0, o_hyp = 0, o_mask = 0, o_rmask = 0;
  int max_groups = 0;
  bool want_hyp = false;
  for (int b = 0; b < B; b++) {
    const Sim3Job& j = jobs[b];
    Sim3Desc& D = w.h_desc[b];
    memset(&D, 0, sizeof(D));
    D.n = j.p->n; D.H = j.H; D.fix_scale = j.p->fix_scale ? 1 : 0; D.min_inliers = j.min_inliers; D.best_in = j.best_in;
    D.n_groups = (j.H + kGroup - 1) / kGroup; D.words = (D.n + 63) / 64;
    D.off_pts = o_pts; D.off_thr = o_thr; D.off_draws = o_draws; D.off_hyp = o_hyp; D.off_mask = o_mask; D.off_rmask = o_rmask;
    D.k1[0] = j.p->fx1; D.k1[1] = j.p->fy1; D.k1[2] = j.p->cx1; D.k1[3] = j.p->cy1;
    D.k2[0] = j.p->fx2; D.k2[1] = j.p->fy2; D.k2[2] = j.p->cx2; D.k2[3] = j.p->cy2;
    o_pts += 6LL * D.n; o_thr += 2LL * D.n; o_draws += 3LL * j.H; o_hyp += j.H; o_mask += (long long)j.H * D.words; o_rmask += D.words;
    max_groups = std::max(max_groups, D.n_groups);
    want_hyp = want_hyp || j.hyp_n_inliers || j.hyp_T12 || j.hyp_masks;
  }
  int rc;
  if ((rc = w.d_desc.reserve(B)) || (rc = w.d_pts.reserve(o_pts)) || (rc = w.d_thr.reserve(o_thr)) || (rc = w.d_draws.reserve(o_draws)) ||
      (rc = w.d_hyp.reserve((size_t)o_hyp * kHypFloats)) || (rc = w.d_counts.reserve(o_hyp)) || (rc = w.d_masks.reserve(o_mask)) ||
      (rc = w.d_rmasks.reserve(o_rmask)) || (rc = w.d_recs.reserve(B)))
    return rc;
  if ((size_t)B > w.tickets_ready) {
    // the tickets start at zero and every launch leaves them at zero: cleared when the buffer is made, never in the call path
    if ((rc = w.d_tickets.reserve(B))) return rc;
    ORBG_HIP(hipMemsetAsync(w.d_tickets.p, 0, w.d_tickets.cap * sizeof(unsigned), st));
    w.tickets_ready = w.d_tickets.cap;
  }
  if (!reuse_pts) {
    w.h_pts.resize(o_pts); w.h_thr.resize(o_thr);
    for (int b = 0; b < B; b++) {
      const orbm_sim3_problem* p = jobs[b].p;
      const Sim3Desc& D = w.h_desc[b];
      const size_t n = D.n;
      memcpy(w.h_pts.data() + D.off_pts, p->X3Dc1, 12 * n); memcpy(w.h_pts.data() + D.off_pts + 3 * n, p->X3Dc2, 12 * n);
      memcpy(w.h_thr.data() + D.off_thr, p->max_err1, 4 * n); memcpy(w.h_thr.data() + D.off_thr + n, p->max_err2, 4 * n);
    }
    ORBG_HIP(hipMemcpyAsync(w.d_pts.p, w.h_pts.data(), (size_t)o_pts * 4, hipMemcpyHostToDevice, st));
    ORBG_HIP(hipMemcpyAsync(w.d_thr.p, w.h_thr.data(), (size_t)o_thr * 4, hipMemcpyHostToDevice, st));
  }
  w.h_draws.resize(o_draws);
  for (int b = 0; b < B; b++) memcpy(w.h_draws.data() + w.h_desc[b].off_draws, jobs[b].draws, 12 * (size_t)jobs[b].H);
  ORBG_HIP(hipMemcpyAsync(w.d_draws.p, w.h_draws.data(), (size_t)o_draws * 4, hipMemcpyHostToDevice, st));
  ORBG_HIP(hipMemcpyAsync(w.d_desc.p, w.h_desc.data(), (size_t)B * sizeof(Sim3Desc), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(sim3_ransac_kernel, dim3(max_groups, B), dim3(kThreads), 0, st, w.d_desc.p, w.d_pts.p, w.d_thr.p, w.d_draws.p, w.d_hyp.p,
                     w.d_counts.p, w.d_masks.p, w.d_tickets.p, w.d_recs.p, w.d_rmasks.p);
  ORBG_HIP(hipGetLastError());
  w.h_recs.resize(B); w.h_rmasks.resize(std::max<long long>(o_rmask, 1));
  ORBG_HIP(hipMemcpyAsync(w.h_recs.data(), w.d_recs.p, (size_t)B * sizeof(Sim3Rec), hipMemcpyDeviceToHost, st));
  ORBG_HIP(hipMemcpyAsync(w.h_rmasks.data(), w.d_rmasks.p, (size_t)o_rmask * 8, hipMemcpyDeviceToHost, st));
  if (want_hyp) {
    w.h_counts.resize(o_hyp); w.h_hyp.resize((size_t)o_hyp * kHypFloats); w.h_masks.resize(std::max<long long>(o_mask, 1));
    ORBG_HIP(hipMemcpyAsync(w.h_counts.data(), w.d_counts.p, (size_t)o_hyp * 4, hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipMemcpyAsync(w.h_hyp.data(), w.d_hyp.p, (size_t)o_hyp * kHypFloats * 4, hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipMemcpyAsync(w.h_masks.data(), w.d_masks.p, (size_t)o_mask * 8, hipMemcpyDeviceToHost, st));
  }
  ORBG_HIP(hipStreamSynchronize(st));
  if (want_hyp)
    for (int b = 0; b < B; b++) {
      const Sim3Job& j = jobs[b];
      const Sim3Desc& D = w.h_desc[b];
      if (j.hyp_n_inliers) memcpy(j.hyp_n_inliers, w.h_counts.data() + D.off_hyp, 4 * (size_t)j.H);
      if (j.hyp_T12)
        for (int h = 0; h < j.H; h++) memcpy(j.hyp_T12 + 16 * (size_t)h, w.h_hyp.data() + (size_t)(D.off_hyp + h) * kHypFloats, 64);
      if (j.hyp_masks) memcpy(j.hyp_masks, w.h_masks.data() + D.off_mask, 8 * (size_t)j.H * D.words);
    }
  return ORBG_OK;
}

}  // namespace

// The state Sim3Solver keeps between iterate() calls (I/Sim3Solver.h:84-101) plus the flat problem
struct orbm_sim3 {
  Sim3Work w;
  bool have_problem = false;
  orbm_sim3_problem prob;
  std::vector<float> X1, X2;
  std::vector<uint32_t> e1, e2;
  int min_inliers = 6, max_its = 300;                 // the header's defaults (I/Sim3Solver.h:46)
  int iterations = 0, best_inliers = 0;               // mnIterations, mnBestInliers
  bool have_best = false;
  float best[kHypFloats];                             // mBestT12, mBestRotation, mBestTranslation, mBestScale
  std::vector<uint8_t> best_mask;                     // mvbBestInliers
};

extern "C" int orbm_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations, int* out) {
  if (!out || n <= 0) return ORBG_BAD_ARG;
  *out = ransac_iterations(n, probability, min_inliers, max_iterations);
  return ORBG_OK;
}

extern "C" int orbm_sim3_resolve_draws(int n, const int32_t* draws, int n_iterations, int32_t* idx) {
  if (n < 3 || n_iterations < 0 || (n_iterations > 0 && (!draws || !idx))) return ORBG_BAD_ARG;
  int rc = check_draws(draws, n_iterations, n);
  if (rc) return rc;
  for (int k = 0; k < n_iterations; k++) sim3_resolve_draws(n, draws[3 * k], draws[3 * k + 1], draws[3 * k + 2], idx + 3 * k);
  return ORBG_OK;
}

extern "C" int orbm_sim3_create(int device, orbm_sim3** out) {
  if (!out) return ORBG_BAD_ARG;
  int rc = select_device(device);
  if (rc) return rc;
  orbm_sim3* h = new orbm_sim3;
  if ((rc = h->w.open(device, "misc"))) { delete h; return rc; }
  *out = h;
  return ORBG_OK;
}

extern "C" int orbm_sim3_destroy(orbm_sim3* h) {
  if (!h) return ORBG_OK;
  h->w.release();
  delete h;
  return ORBG_OK;
}

extern "C" int orbm_sim3_set_stream(orbm_sim3* h, void* hip_stream) {
  if (!h) return ORBG_BAD_ARG;
  int rc = select_device(h->w.device);
  if (rc) return rc;
  return orbg::swap_stream(&h->w.stream, &h->w.ext_stream, hip_stream, "misc");
}

extern "C" int orbm_sim3_set_problem(orbm_sim3* h, const orbm_sim3_problem* p) {
  if (!h) return ORBG_BAD_ARG;
  int rc = check_problem(p);
  if (rc) return rc;
  const size_t n = p->n;
  h->X1.assign(p->X3Dc1, p->X3Dc1 + 3 * n); h->X2.assign(p->X3Dc2, p->X3Dc2 + 3 * n);
  h->e1.assign(p->max_err1, p->max_err1 + n); h->e2.assign(p->max_err2, p->max_err2 + n);
  memset(&h->prob, 0, sizeof(h->prob));
  memcpy(&h->prob, p, sizeof(orbm_sim3_problem));
  h->prob.X3Dc1 = h->X1.data(); h->prob.X3Dc2 = h->X2.data(); h->prob.max_err1 = h->e1.data(); h->prob.max_err2 = h->e2.data();
  h->have_problem = true;
  h->w.pts_resident = -1;
  h->iterations = 0; h->best_inliers = 0; h->have_best = false;
  h->best_mask.assign(n, 0);
  // the constructor ends with SetRansacParameters() at its defaults, S/Sim3Solver.cc:127, I/Sim3Solver.h:46
  h->min_inliers = 6;
  h->max_its = n > 0 ? ransac_iterations((int)n, 0.99, 6, 300) : 1;
  return ORBG_OK;
}

extern "C" int orbm_sim3_set_ransac_parameters(orbm_sim3* h, double probability, int min_inliers, int max_iterations) {
  if (!h || !h->have_problem) return ORBG_BAD_ARG;
  h->min_inliers = min_inliers;
  h->max_its = h->prob.n > 0 ? ransac_iterations(h->prob.n, probability, min_inliers, max_iterations) : std::max(1, max_iterations);
  h->iterations = 0;                                   // :156; mnBestInliers and the best hypothesis are NOT reset there
  return ORBG_OK;
}

namespace {
void fill_result(orbm_sim3_result* r, const float* hyp) {
  memcpy(r->T12, hyp, 64); memcpy(r->R, hyp + 16, 36); memcpy(r->t, hyp + 25, 12); r->s = hyp[28];
}
void unpack_mask(const unsigned long long* words, int n, uint8_t* out) {
  for (int i = 0; i < n; i++) out[i] = (uint8_t)((words[i >> 6] >> (i & 63)) & 1ULL);
}
void clear_result(orbm_sim3_result* r, int n) {
  r->no_more = 0; r->converged = 0; r->n_inliers = 0; r->iterations_done = 0; r->improved_in_this_call = 0; r->best_iteration = -1;
  r->iterations_run = 0; r->have_best = 0;
  memset(r->T12, 0, sizeof(r->T12)); memset(r->R, 0, sizeof(r->R)); memset(r->t, 0, sizeof(r->t)); r->s = 0.0f;
  if (r->inliers && n > 0) memset(r->inliers, 0, n);
}
}  // namespace

extern "C" int orbm_sim3_iterate(orbm_sim3* h, int n_iterations, const int32_t* draws, orbm_sim3_result* r) {
  if (!h || !h->have_problem || !r || r->struct_size < sizeof(orbm_sim3_result) || n_iterations < 0) return ORBG_BAD_ARG;
  const int n = h->prob.n;
  clear_result(r, n);
  r->iterations_done = h->iterations;
  if (n < h->min_inliers) { r->no_more = 1; return ORBG_OK; }                       // :165-169, no launch
  const int H = std::max(0, std::min(n_iterations, h->max_its - h->iterations));     // :179
  int rc = check_draws(draws, H, n);
  if (rc) return rc;
  if (H > 0) {
    if ((rc = select_device(h->w.device))) return rc;
    std::vector<Sim3Job> jobs(1);
    jobs[0] = Sim3Job{&h->prob, H, h->min_inliers, h->best_inliers, draws, r->hyp_n_inliers, r->hyp_T12, r->hyp_masks};
    const bool reuse = h->w.pts_resident == 0;
    if ((rc = launch(h->w, jobs, reuse))) return rc;
    h->w.pts_resident = 0;
    const Sim3Rec& rec = h->w.h_recs[0];
    const int run = rec.converged ? rec.index + 1 : H;
    h->iterations += run;
    r->iterations_run = run;
    if (rec.index >= 0) {
      h->best_inliers = rec.count; h->have_best = true;
      memcpy(h->best, rec.hyp, sizeof(h->best));
      unpack_mask(h->w.h_rmasks.data(), n, h->best_mask.data());
      r->improved_in_this_call = 1;
      r->best_iteration = h->iterations - run + rec.index;
    }
    r->converged = rec.converged;
  }
  r->iterations_done = h->iterations;
  r->n_inliers = h->best_inliers;
  r->have_best = h->have_best ? 1 : 0;
  if (h->have_best) {
    fill_result(r, h->best);
    if (r->inliers && n > 0) memcpy(r->inliers, h->best_mask.data(), n);
  }
  if (!r->converged && h->iterations >= h->max_its) r->no_more = 1;                  // :236-237 (not reached on convergence)
  return ORBG_OK;
}

namespace {
Sim3Work& batch_work() { static thread_local Sim3Work w; return w; }
}

extern "C" int orbm_sim3_solve_batch(int device, const orbm_sim3_problem* problems, int B, const orbm_sim3_params* params,
                                     const int32_t* const* draws, orbm_sim3_result* results) {
  if (B < 0 || (B > 0 && (!problems || !params || !draws || !results))) return ORBG_BAD_ARG;
  // every argument is checked, and the device, before any result is written: a call that fails leaves `results` as it found them
  std::vector<Sim3Job> jobs;
  std::vector<int> job_of(B, -1), max_its(B, 0);
  int rc;
  for (int b = 0; b < B; b++) {
    if ((rc = check_problem(&problems[b]))) return rc;
    if (results[b].struct_size < sizeof(orbm_sim3_result)) return ORBG_BAD_ARG;
    const int n = problems[b].n;
    if (n < params[b].min_inliers) continue;                      // :165-169: bNoMore, no launch
    if (n < 1) return ORBG_BAD_ARG;
    const int H = max_its[b] = ransac_iterations(n, params[b].probability, params[b].min_inliers, params[b].max_iterations);
    if ((rc = check_draws(draws[b], H, n))) return rc;            // (also refuses 1 <= n < 3: no minimal set can be drawn)
    job_of[b] = (int)jobs.size();
    jobs.push_back(Sim3Job{&problems[b], H, params[b].min_inliers, 0, draws[b], results[b].hyp_n_inliers, results[b].hyp_T12, results[b].hyp_masks});
  }
  rc = select_device(device);
  if (rc) return rc;
  for (int b = 0; b < B; b++) {
    clear_result(&results[b], problems[b].n);
    if (job_of[b] < 0) results[b].no_more = 1;
  }
  if (jobs.empty()) return ORBG_OK;
  Sim3Work& w = batch_work();
  if ((rc = w.open(device, "misc"))) return rc;
  if ((rc = launch(w, jobs, false))) return rc;
  for (int b = 0; b < B; b++) {
    if (job_of[b] < 0) continue;
    const Sim3Rec& rec = w.h_recs[job_of[b]];
    orbm_sim3_result* r = &results[b];
    const int n = problems[b].n;
    r->converged = rec.converged;
    r->iterations_run = r->iterations_done = rec.converged ? rec.index + 1 : max_its[b];
    if (rec.index >= 0) {
      r->improved_in_this_call = 1; r->best_iteration = rec.index; r->have_best = 1; r->n_inliers = rec.count;
      fill_result(r, rec.hyp);
      if (r->inliers) unpack_mask(w.h_rmasks.data() + w.h_desc[job_of[b]].off_rmask, n, r->inliers);
    }
    if (!r->converged) r->no_more = 1;
  }
  return ORBG_OK;
}
