// TwoViewReconstruction::Reconstruct (S/TwoViewReconstruction.cc:39-127) and everything it calls, for gfx950: FindHomography,
// FindFundamental, ComputeH21, ComputeF21, CheckHomography, CheckFundamental, Normalize, ReconstructF, ReconstructH, DecomposeE,
// CheckRT and Triangulate.  Two launches on one stream, no host round trip between them.
//
// Launch 1, tv_ransac_kernel.  Grid = 2 * ceil(iterations / kGroup) workgroups of kGroup = 32 lanes: the first half holds the
// homography hypotheses, the second half the fundamental-matrix ones, so a workgroup never diverges between the two models.
//   Phase A  one lane per hypothesis: eight raw draws -> the minimal set (resolve_draws.hpp), the design matrix row by row, A^T A
//            in float64, its 9 x 9 cyclic Jacobi in LDS (two 81-entry float64 matrices per lane, [entry][lane]: conflict-free), the
//            null vector, then H21i / H12i or the rank-2 F21i in the reference's types.
//   Phase B  the same lane walks ALL matches in match order: the matches pass through LDS in tiles of kTile and are read as
//            broadcasts; `score += th - chiSquare` is the reference's left-to-right float sum, the 64 inlier bits of a mask word
//            come from the same walk.  No reduction across lanes exists, so the score has the serial loop's bits.
//   Phase C  the workgroup that takes the last ticket replays `currentScore > score` over the scores in iteration order (first
//            iteration with the strictly largest score, from score = 0: a zero or NaN score never wins), forms SH, SF and RH, and
//            one lane writes the motion hypotheses of the chosen model: ReconstructH's eight (:588-690) or DecomposeE's four.
// Launch 2, tv_check_rt_kernel.  Grid = 8 workgroups of 256 lanes, one per motion hypothesis, lanes over matches: CheckRT for every
// inlier, nGood as an integer sum, the parallax from an exact rank selection of sorted[min(50, size - 1)].  The last ticket applies
// the final decision of ReconstructF (:504-574) or ReconstructH (:693-735) and scatters vP3D / vbTriangulated by keypoint index.
// Every reduction is an integer sum, a max or a rank count: two runs give the same bits.
//
// Arithmetic.  The reference's cv::Mat are CV_32F; what OpenCV does INSIDE a call on them is not part of the reference's source.
// The choices made here (tests/two_view_model.py restates the same ones and is itself compared with a float64 evaluation); T-2 / T-3
// / T-4 are C-2 / C-3 / C-4 of sim3.hip, T-7 is N-5 and T-1's null vector is N-8 of newpoints.hip:
//   T-1  cv::SVDecomp(A) of the 16 x 9 / 8 x 9 design matrix, vt.row(8): OpenCV's float one-sided Jacobi is NOT pinned to the bit.
//        Here the design matrix is float32 as written; S = A^T A is accumulated in float64 row by row; the null vector is the
//        eigenvector of the smallest eigenvalue of S (first one on a tie) by cyclic Jacobi in float64 -- sweep order (p, q) with p < q
//        ascending, tau = (S_qq - S_pp) / (2 S_pq), t = sgn(tau) / (|tau| + sqrt(1 + tau^2)), columns, then rows, then the vectors;
//        stop when sum(off^2) is not above 1e-28 * sum(diag^2), or after 60 sweeps -- rounded once to float32.  Its sign is whatever the
//        rotations give: H and H^-1 are homogeneous, CheckFundamental squares num, and {R1, R2} x {t, -t} is the same SET.
//   T-2  cv::Mat products (T2inv * Hn * T1, T2^T * Fn * T1, u * diag(w) * vt, K^T * F21 * K, invK * H21 * K, u * W * vt, s * U * Rp * Vt,
//        U * tp, K * [R|t], -R^T * t, R * p + t): cv::gemm accumulates each entry in DOUBLE in k order, applies alpha / beta in double
//        and rounds once to float; a product of three matrices rounds the intermediate matrix to float.
//   T-3  Mat::dot and cv::norm accumulate double products of the float entries in storage order.
//   T-4  a matrix scaled by a scalar (t / norm(t), tp *= d1 - d3, x3D / x3D(3)): the scalar is formed in double, rounded to float, and
//        the entries are multiplied in float.
//   T-5  the 3 x 3 cv::SVDecomp / cv::SVD::compute (rank-2 enforcement in ComputeF21, DecomposeE, ReconstructH's A): eigenvectors V of
//        M^T M by the Jacobi of T-1 in float64, eigenvalues sorted descending (stable), w = sqrt(max(lambda, 0)), u_i = M v_i / w_i;
//        where the third singular value is zero by construction (ComputeF21, DecomposeE) u_2 = u_0 x u_1, in ReconstructH u_2 =
//        M v_2 / w_2 so that det(U) det(Vt) is the sign of det(A).  U, w, V are rounded once to float32.
//   T-6  H21i.inv(), T2.inv(), K.inv(): cofactors and determinant in double, d = 1 / det, each entry (cofactor * d) rounded once
//        (N-4 of newpoints.hip).  A singular matrix gives non-finite entries, every chi-square is NaN, the score is NaN and never wins.
//   T-7  kp.pt.x * P.row(2) - P.row(0) in Triangulate: float multiply, float subtract per entry.  The 4 x 4 null vector goes through
//        null_vector4.hpp.
//   T-8  scalar C++ expressions keep the reference's types: float throughout, double where a double literal or a double-returning
//        call takes part.  (float)(1.0 / (double)x) for a float x equals the correctly rounded float quotient 1.0f / x (double
//        rounding is innocuous for a quotient of floats), so 1.0 / (...) in the two checkers and CheckRT is one float division.
//        cv::determinant's sign and acos are evaluated in double; parallax = (float)((double)((float)acos((double)c) * 180.0f) / pi).
// Built with -ffp-contract=off and correctly rounded float divide / sqrt, like the rest of the library.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "null_vector4.hpp"
#include "resolve_draws.hpp"

using orbg::select_device;

namespace {

constexpr int kGroup = 32;        // hypotheses per workgroup, one lane each
constexpr int kTile = 256;        // matches staged in LDS at a time (a multiple of 64: a mask word never straddles two tiles)
constexpr int kSweeps = 60;
constexpr int kRtThreads = 256;
constexpr int kMotions = 8;
constexpr int kHypFloats = 18;    // per hypothesis in global memory: H21i[9] H12i[9] / F21i[9], 9 unused
constexpr int kMaxMatches = ORBI_TWO_VIEW_MAX_MATCHES;
typedef unsigned long long u64;

struct TvParams {                 // by value to both kernels
  int N, n1, H, nG, words;
  float fx, fy, cx, cy, sigma;
  float T1[9], T2[9], T2inv[9];
};

struct TvRec {                    // what the host reads back; lives at the head of the output buffer
  int success, model, bestH, bestF, n_inliers, n_motions, best_motion, h_degenerate;
  float SH, SF;
  float H21[9], F21[9], R21[9], t21[3];
  int nGood[kMotions];
  float parallax[kMotions];
  float R[kMotions][9];
  float t[kMotions][3];
};

// ---------------------------------------------------------------------------------------------- small matrices (T-2, T-5, T-6)

__host__ __device__ __forceinline__ double dot3d(float a0, float a1, float a2, float b0, float b1, float b2) {
  return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// c = a * b, 3 x 3 row-major (T-2)
__host__ __device__ __forceinline__ void mul3(const float* a, const float* b, float* c) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) c[i * 3 + j] = (float)dot3d(a[i * 3], a[i * 3 + 1], a[i * 3 + 2], b[j], b[3 + j], b[6 + j]);
}

__host__ __device__ __forceinline__ void transpose3(const float* a, float* t) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) t[i * 3 + j] = a[j * 3 + i];
}

__host__ __device__ __forceinline__ double det3d(const float* m) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

// T-6
__host__ __device__ __forceinline__ void inv3(const float* m, float* o) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  const double det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
  const double id = 1.0 / det;
  o[0] = (float)((e * i - f * h) * id); o[1] = (float)((c * h - b * i) * id); o[2] = (float)((b * f - c * e) * id);
  o[3] = (float)((f * g - d * i) * id); o[4] = (float)((a * i - c * g) * id); o[5] = (float)((c * d - a * f) * id);
  o[6] = (float)((d * h - e * g) * id); o[7] = (float)((b * g - a * h) * id); o[8] = (float)((a * e - b * d) * id);
}

// The Jacobi of T-1 on a symmetric 3 x 3 held in registers (compile-time indices only)
__device__ __forceinline__ void jacobi3(double (&S)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSweeps; sweep++) {
    double off = 0, diag = 0;
#pragma unroll
    for (int p = 0; p < 3; p++) {
      diag += S[p][p] * S[p][p];
#pragma unroll
      for (int q = p + 1; q < 3; q++) off += S[p][q] * S[p][q];
    }
    if (!(off > 1e-28 * diag)) break;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 3; q++) {
        if (S[p][q] == 0.0) continue;
        const double tau = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
#pragma unroll
        for (int k = 0; k < 3; k++) { const double a = S[k][p], b = S[k][q]; S[k][p] = cs * a - sn * b; S[k][q] = sn * a + cs * b; }
#pragma unroll
        for (int k = 0; k < 3; k++) { const double a = S[p][k], b = S[q][k]; S[p][k] = cs * a - sn * b; S[q][k] = sn * a + cs * b; }
#pragma unroll
        for (int k = 0; k < 3; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = cs * a - sn * b; V[k][q] = sn * a + cs * b; }
      }
  }
}

// T-5.  M row-major float; U, V row-major float (columns are the singular vectors), w descending.
__device__ void svd3(const float* M, bool complete, float* U, float* w, float* V) {
  double S[3][3], E[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double acc = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) acc += (double)M[k * 3 + i] * (double)M[k * 3 + j];
      S[i][j] = acc;
    }
  jacobi3(S, E);
  double l[3] = {S[0][0], S[1][1], S[2][2]};
#define TV_SORT2(a, b)                                                                                         \
  if (l[a] < l[b]) {                                                                                           \
    double x = l[a]; l[a] = l[b]; l[b] = x;                                                                    \
    _Pragma("unroll") for (int k = 0; k < 3; k++) { x = E[k][a]; E[k][a] = E[k][b]; E[k][b] = x; }             \
  }
  TV_SORT2(0, 1) TV_SORT2(1, 2) TV_SORT2(0, 1)
#undef TV_SORT2
  double u[3][3], sg[3];           // u[column][row]
#pragma unroll
  for (int c = 0; c < 3; c++) {
    sg[c] = sqrt(l[c] > 0 ? l[c] : 0.0);
#pragma unroll
    for (int r = 0; r < 3; r++)
      u[c][r] = (((double)M[r * 3] * E[0][c] + (double)M[r * 3 + 1] * E[1][c]) + (double)M[r * 3 + 2] * E[2][c]) / sg[c];
  }
  if (complete) {
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    w[c] = (float)sg[c];
#pragma unroll
    for (int r = 0; r < 3; r++) { U[r * 3 + c] = (float)u[c][r]; V[r * 3 + c] = (float)E[r][c]; }
  }
}

// ---------------------------------------------------------------------------------------------- launch 1

// T-1 on a lane's 9 x 9 in LDS: S and V are [81][kGroup], entry (i, j) at [i * 9 + j][lane]; v = the null vector
__device__ void null_vector9(double (*S)[kGroup], double (*V)[kGroup], int lane, float* v) {
  for (int i = 0; i < 81; i++) V[i][lane] = (i / 9 == i % 9) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSweeps; sweep++) {
    double off = 0, diag = 0;
    for (int p = 0; p < 9; p++) {
      const double d = S[p * 10][lane];
      diag += d * d;
      for (int q = p + 1; q < 9; q++) { const double o = S[p * 9 + q][lane]; off += o * o; }
    }
    if (!(off > 1e-28 * diag)) break;
    for (int p = 0; p < 9; p++)
      for (int q = p + 1; q < 9; q++) {
        const double spq = S[p * 9 + q][lane];
        if (spq == 0.0) continue;
        const double tau = (S[q * 10][lane] - S[p * 10][lane]) / (2.0 * spq);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
        for (int k = 0; k < 9; k++) {
          const double a = S[k * 9 + p][lane], b = S[k * 9 + q][lane];
          S[k * 9 + p][lane] = cs * a - sn * b; S[k * 9 + q][lane] = sn * a + cs * b;
        }
        for (int k = 0; k < 9; k++) {
          const double a = S[p * 9 + k][lane], b = S[q * 9 + k][lane];
          S[p * 9 + k][lane] = cs * a - sn * b; S[q * 9 + k][lane] = sn * a + cs * b;
        }
        for (int k = 0; k < 9; k++) {
          const double a = V[k * 9 + p][lane], b = V[k * 9 + q][lane];
          V[k * 9 + p][lane] = cs * a - sn * b; V[k * 9 + q][lane] = sn * a + cs * b;
        }
      }
  }
  int m = 0;
  double smallest = S[0][lane];
  for (int i = 1; i < 9; i++) { const double d = S[i * 10][lane]; if (d < smallest) { smallest = d; m = i; } }
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] = (float)V[k * 9 + m][lane];
}

// one design-matrix row into the upper triangle of S (45 accumulators in registers, row-major over i <= j)
__device__ __forceinline__ void ata_add(double (&acc)[45], const float (&a)[9]) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = i; j < 9; j++) { acc[k] += (double)a[i] * (double)a[j]; k++; }
}

// publish this workgroup's stores and take a ticket; true in the workgroup that took the last of `total` (sim3.hip, phase C: every
// wavefront drains its own stores before the barrier, the release fence and its wait stand before the ticket, the acquire fence
// and its wait before the barrier that lets the other lanes read)
__device__ bool last_ticket(unsigned* ticket, int total, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned before = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = before == (unsigned)(total - 1);
    if (last) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

__device__ __forceinline__ void scale3(float* t, float a) { t[0] = t[0] * a; t[1] = t[1] * a; t[2] = t[2] * a; }

// t / cv::norm(t) (T-3, T-4)
__device__ __forceinline__ void normalise3(float* t) {
  const double nrm = sqrt(((double)t[0] * t[0] + (double)t[1] * t[1]) + (double)t[2] * t[2]);
  scale3(t, (float)(1.0 / nrm));
}

// DecomposeE, :913-933, and the four hypotheses of ReconstructF, :484-502
__device__ void motions_F(const TvParams& P, TvRec* rec) {
  const float K[9] = {P.fx, 0.f, P.cx, 0.f, P.fy, P.cy, 0.f, 0.f, 1.f};
  float Kt[9], tmp[9], E[9], U[9], w[3], V[9], Vt[9];
  transpose3(K, Kt);
  mul3(Kt, rec->F21, tmp); mul3(tmp, K, E);
  svd3(E, true, U, w, V);
  transpose3(V, Vt);
  float t[3] = {U[2], U[5], U[8]};
  normalise3(t);
  float uW[9], uWt[9], R1[9], R2[9];
#pragma unroll
  for (int i = 0; i < 3; i++) {    // u * W = [u1, -u0, u2], u * W^t = [-u1, u0, u2] (exact)
    uW[i * 3] = U[i * 3 + 1]; uW[i * 3 + 1] = -U[i * 3]; uW[i * 3 + 2] = U[i * 3 + 2];
    uWt[i * 3] = -U[i * 3 + 1]; uWt[i * 3 + 1] = U[i * 3]; uWt[i * 3 + 2] = U[i * 3 + 2];
  }
  mul3(uW, Vt, R1); mul3(uWt, Vt, R2);
  if (det3d(R1) < 0) { for (int k = 0; k < 9; k++) R1[k] = -R1[k]; }
  if (det3d(R2) < 0) { for (int k = 0; k < 9; k++) R2[k] = -R2[k]; }
  for (int m = 0; m < 4; m++) {
    for (int k = 0; k < 9; k++) rec->R[m][k] = (m & 1) ? R2[k] : R1[k];
    for (int k = 0; k < 3; k++) rec->t[m][k] = (m & 2) ? -t[k] : t[k];
  }
  rec->n_motions = 4;
}

// ReconstructH up to its CheckRT loop, :588-690
__device__ void motions_H(const TvParams& P, TvRec* rec) {
  const float K[9] = {P.fx, 0.f, P.cx, 0.f, P.fy, P.cy, 0.f, 0.f, 1.f};
  float invK[9], tmp[9], A[9], U[9], w[3], V[9], Vt[9];
  inv3(K, invK);
  mul3(invK, rec->H21, tmp); mul3(tmp, K, A);
  svd3(A, false, U, w, V);
  transpose3(V, Vt);
  const float s = (float)(det3d(U) * det3d(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) { rec->h_degenerate = 1; rec->n_motions = 0; return; }
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  for (int m = 0; m < 8; m++) {
    const int i = m & 3;
    float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3];
    float f;                       // tp *= d1 -+ d3
    if (m < 4) {
      Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
      f = d1 - d3; tp[0] = x1[i]; tp[1] = 0.f; tp[2] = -x3[i];
    } else {
      Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi;
      f = d1 + d3; tp[0] = x1[i]; tp[1] = 0.f; tp[2] = x3[i];
    }
    scale3(tp, f);
    float M1[9], R[9], t[3];
    for (int r = 0; r < 3; r++)    // gemm(U, Rp, alpha = s), then * Vt (T-2)
      for (int c = 0; c < 3; c++) M1[r * 3 + c] = (float)((double)s * dot3d(U[r * 3], U[r * 3 + 1], U[r * 3 + 2], Rp[c], Rp[3 + c], Rp[6 + c]));
    mul3(M1, Vt, R);
    for (int r = 0; r < 3; r++) t[r] = (float)dot3d(U[r * 3], U[r * 3 + 1], U[r * 3 + 2], tp[0], tp[1], tp[2]);
    normalise3(t);
    for (int k = 0; k < 9; k++) rec->R[m][k] = R[k];
    for (int k = 0; k < 3; k++) rec->t[m][k] = t[k];
  }
  rec->n_motions = 8;
}

// in: u1[N] v1[N] u2[N] v2[N] (mvKeys of the matches) pn1x[N] pn1y[N] pn2x[N] pn2y[N] (vPn1 / vPn2 of the matches)
__global__ __launch_bounds__(kGroup) void tv_ransac_kernel(TvParams P, const float* __restrict__ in, const int* __restrict__ draws,
                                                           float* __restrict__ hyp, float* __restrict__ scores, u64* __restrict__ masks,
                                                           int* __restrict__ sets, unsigned* __restrict__ tickets, TvRec* __restrict__ rec) {
  __shared__ double sS[81][kGroup];
  __shared__ double sV[81][kGroup];
  __shared__ float sM[4][kTile];
  __shared__ float sBest[kGroup];
  __shared__ int sIdx[kGroup];
  __shared__ int sFlag;
  const int lane = threadIdx.x;
  const bool isF = (int)blockIdx.x >= P.nG;
  const int it = (isF ? (int)blockIdx.x - P.nG : (int)blockIdx.x) * kGroup + lane;
  const bool live = it < P.H;
  const int N = P.N;
  const int row = isF ? P.H + it : it;   // this hypothesis among the 2 H
  float M[9], Mi[9];                     // H21i / F21i, H12i

  // ---- phase A
  if (live) {
    int r[8], idx[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = draws[8 * (size_t)it + j];
    orbg::resolve_draws<8>(N, r, idx);
    if (!isF) {
#pragma unroll
      for (int j = 0; j < 8; j++) sets[8 * (size_t)it + j] = idx[j];
    }
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; k++) acc[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
      int m = idx[0];                    // (compile-time indices only)
#pragma unroll
      for (int k = 1; k < 8; k++) m = j == k ? idx[k] : m;
      const float u1 = in[4 * (size_t)N + m], v1 = in[5 * (size_t)N + m], u2 = in[6 * (size_t)N + m], v2 = in[7 * (size_t)N + m];
      if (!isF) {                        // ComputeH21, :244-262
        const float a0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float a1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        ata_add(acc, a0); ata_add(acc, a1);
      } else {                           // ComputeF21, :286-294
        const float a[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        ata_add(acc, a);
      }
    }
    {
      int k = 0;
#pragma unroll
      for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = i; j < 9; j++) { sS[i * 9 + j][lane] = acc[k]; sS[j * 9 + i][lane] = acc[k]; k++; }
    }
    float h[9];
    null_vector9(sS, sV, lane, h);
    float tmp[9];
    if (!isF) {                          // :164-166
      mul3(P.T2inv, h, tmp); mul3(tmp, P.T1, M);
      inv3(M, Mi);
    } else {                             // :301-307, :217
      float U[9], w[3], V[9], Vt[9], UW[9], Fn[9], T2t[9];
      svd3(h, true, U, w, V);
      w[2] = 0.f;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) UW[i * 3 + j] = U[i * 3 + j] * w[j];
      transpose3(V, Vt);
      mul3(UW, Vt, Fn);
      transpose3(P.T2, T2t);
      mul3(T2t, Fn, tmp); mul3(tmp, P.T1, M);
#pragma unroll
      for (int k = 0; k < 9; k++) Mi[k] = 0.f;
    }
    float* out = hyp + (size_t)row * kHypFloats;
#pragma unroll
    for (int k = 0; k < 9; k++) { out[k] = M[k]; out[9 + k] = Mi[k]; }
  }

  // ---- phase B: CheckHomography (:310-393) / CheckFundamental (:395-473) over all matches, in match order
  const float th = isF ? 3.841f : 5.991f, thScore = 5.991f;
  const float invSigmaSquare = 1.0f / (P.sigma * P.sigma);
  float score = 0.f;
  u64 word = 0;
  u64* mrow = masks + (size_t)row * P.words;
  for (int t0 = 0; t0 < N; t0 += kTile) {
    const int tn = min(kTile, N - t0);
    __syncthreads();
    for (int i = lane; i < tn; i += kGroup) {
      sM[0][i] = in[t0 + i]; sM[1][i] = in[(size_t)N + t0 + i]; sM[2][i] = in[2 * (size_t)N + t0 + i]; sM[3][i] = in[3 * (size_t)N + t0 + i];
    }
    __syncthreads();
    if (!live) continue;
    for (int i = 0; i < tn; i++) {
      const float u1 = sM[0][i], v1 = sM[1][i], u2 = sM[2][i], v2 = sM[3][i];
      bool bIn = true;
      if (!isF) {
        const float w2in1inv = 1.0f / (Mi[6] * u2 + Mi[7] * v2 + Mi[8]);
        const float u2in1 = (Mi[0] * u2 + Mi[1] * v2 + Mi[2]) * w2in1inv;
        const float v2in1 = (Mi[3] * u2 + Mi[4] * v2 + Mi[5]) * w2in1inv;
        const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > th) bIn = false; else score += th - chiSquare1;
        const float w1in2inv = 1.0f / (M[6] * u1 + M[7] * v1 + M[8]);
        const float u1in2 = (M[0] * u1 + M[1] * v1 + M[2]) * w1in2inv;
        const float v1in2 = (M[3] * u1 + M[4] * v1 + M[5]) * w1in2inv;
        const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th) bIn = false; else score += th - chiSquare2;
      } else {
        const float a2 = M[0] * u1 + M[1] * v1 + M[2];
        const float b2 = M[3] * u1 + M[4] * v1 + M[5];
        const float c2 = M[6] * u1 + M[7] * v1 + M[8];
        const float num2 = a2 * u2 + b2 * v2 + c2;
        const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > th) bIn = false; else score += thScore - chiSquare1;
        const float a1 = M[0] * u2 + M[3] * v2 + M[6];
        const float b1 = M[1] * u2 + M[4] * v2 + M[7];
        const float c1 = M[2] * u2 + M[5] * v2 + M[8];
        const float num1 = a1 * u1 + b1 * v1 + c1;
        const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th) bIn = false; else score += thScore - chiSquare2;
      }
      const int gi = t0 + i;
      if (bIn) word |= 1ULL << (gi & 63);
      if ((gi & 63) == 63 || gi == N - 1) { mrow[gi >> 6] = word; word = 0; }
    }
  }
  if (live) scores[row] = score;

  // ---- phase C
  if (!last_ticket(&tickets[0], 2 * P.nG, &sFlag)) return;
  int best[2];
  float bestS[2];
  for (int k = 0; k < 2; k++) {          // :170 / :221 over the scores in iteration order
    float s = 0.f;
    int bi = -1;
    for (int i = lane; i < P.H; i += kGroup) {
      const float c = scores[k * P.H + i];
      if (c > s) { s = c; bi = i; }
    }
    __syncthreads();
    sBest[lane] = s; sIdx[lane] = bi;
    __syncthreads();
    s = 0.f; bi = -1;
    for (int l = 0; l < kGroup; l++) {
      const float c = sBest[l];
      const int ci = sIdx[l];
      if (ci >= 0 && (c > s || (c == s && ci < bi))) { s = c; bi = ci; }
    }
    best[k] = bi; bestS[k] = s;
  }
  if (lane != 0) return;
  const float SH = bestS[0], SF = bestS[1];
  rec->success = 0; rec->bestH = best[0]; rec->bestF = best[1]; rec->SH = SH; rec->SF = SF;
  rec->n_motions = 0; rec->best_motion = -1; rec->h_degenerate = 0; rec->n_inliers = 0;
  for (int k = 0; k < 9; k++) {
    rec->H21[k] = best[0] >= 0 ? hyp[(size_t)best[0] * kHypFloats + k] : 0.f;
    rec->F21[k] = best[1] >= 0 ? hyp[(size_t)(P.H + best[1]) * kHypFloats + k] : 0.f;
    rec->R21[k] = 0.f;
  }
  for (int k = 0; k < 3; k++) rec->t21[k] = 0.f;
  for (int m = 0; m < kMotions; m++) {
    rec->nGood[m] = 0; rec->parallax[m] = 0.f;
    for (int k = 0; k < 9; k++) rec->R[m][k] = 0.f;
    for (int k = 0; k < 3; k++) rec->t[m][k] = 0.f;
  }
  int model = 0;
  if (!(SH + SF == 0.f)) {               // :111-117
    const float RH = SH / (SH + SF);
    model = (double)RH > 0.50 ? 1 : 2;
  }
  rec->model = model;
  if (model == 0) return;
  const u64* brow = masks + (size_t)(model == 1 ? best[0] : P.H + best[1]) * P.words;
  int n_in = 0;
  for (int wd = 0; wd < P.words; wd++) n_in += __popcll(brow[wd]);
  rec->n_inliers = n_in;
  if (model == 1) motions_H(P, rec); else motions_F(P, rec);
}

// ---------------------------------------------------------------------------------------------- launch 2

// CheckRT, :802-911, one workgroup per motion hypothesis; the last one to finish applies :504-574 / :693-735.
// flags: bit 0 = counted in nGood (vP3D written), bit 1 = vbGood
__global__ __launch_bounds__(kRtThreads) void tv_check_rt_kernel(TvParams P, const float* __restrict__ in, const int* __restrict__ idx1,
                                                                 const u64* __restrict__ masks, TvRec* __restrict__ rec,
                                                                 uint8_t* __restrict__ flags, float* __restrict__ p3d,
                                                                 unsigned* __restrict__ tickets, float* __restrict__ outP3D,
                                                                 uint8_t* __restrict__ outTri) {
  __shared__ float sCos[kMaxMatches];
  __shared__ uint8_t sCnt[kMaxMatches];
  __shared__ int sRed[kRtThreads];
  __shared__ float sSel;
  __shared__ int sFlag, sChosen;
  const int tid = threadIdx.x, m = blockIdx.x, N = P.N;
  const int nm = rec->n_motions, model = rec->model;
  if (m < nm) {
    float R[9], t[3], P2[12], O2[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rec->R[m][k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = rec->t[m][k];
    const float K[9] = {P.fx, 0.f, P.cx, 0.f, P.fy, P.cy, 0.f, 0.f, 1.f};
#pragma unroll
    for (int i = 0; i < 3; i++) {        // P2 = K * [R|t], O2 = -R^t * t (T-2)
#pragma unroll
      for (int j = 0; j < 3; j++) P2[i * 4 + j] = (float)dot3d(K[i * 3], K[i * 3 + 1], K[i * 3 + 2], R[j], R[3 + j], R[6 + j]);
      P2[i * 4 + 3] = (float)dot3d(K[i * 3], K[i * 3 + 1], K[i * 3 + 2], t[0], t[1], t[2]);
      O2[i] = (float)(-1.0 * dot3d(R[i], R[3 + i], R[6 + i], t[0], t[1], t[2]));
    }
    const float P1[12] = {P.fx, 0.f, P.cx, 0.f, 0.f, P.fy, P.cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    const float th2 = (float)(4.0 * (double)(P.sigma * P.sigma));
    const u64* brow = masks + (size_t)(model == 1 ? rec->bestH : P.H + rec->bestF) * P.words;
    int cnt = 0;
    for (int i = tid; i < N; i += kRtThreads) {
      uint8_t fl = 0;
      float cosParallax = 0.f;
      if ((brow[i >> 6] >> (i & 63)) & 1ULL) {
        const float x1 = in[i], y1 = in[(size_t)N + i], x2 = in[2 * (size_t)N + i], y2 = in[3 * (size_t)N + i];
        float A[4][4];                   // Triangulate, :738-751 (T-7)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          A[0][j] = x1 * P1[8 + j] - P1[j];
          A[1][j] = y1 * P1[8 + j] - P1[4 + j];
          A[2][j] = x2 * P2[8 + j] - P2[j];
          A[3][j] = y2 * P2[8 + j] - P2[4 + j];
        }
        double S[4][4], v[4];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) {
            double acc = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) acc += (double)A[k][a] * (double)A[k][b];
            S[a][b] = acc;
          }
        orbg::null_vector4(S, v);
        const float inv = (float)(1.0 / (double)(float)v[3]);     // T-4
        const float p[3] = {(float)v[0] * inv, (float)v[1] * inv, (float)v[2] * inv};
        bool go = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        float p2[3] = {0.f, 0.f, 0.f};
        if (go) {
          const float n2[3] = {p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]};     // normal1 = p - 0 = p
          const float dist1 = (float)sqrt(((double)p[0] * p[0] + (double)p[1] * p[1]) + (double)p[2] * p[2]);
          const float dist2 = (float)sqrt(((double)n2[0] * n2[0] + (double)n2[1] * n2[1]) + (double)n2[2] * n2[2]);
          const double dt = ((double)p[0] * n2[0] + (double)p[1] * n2[1]) + (double)p[2] * n2[2];
          cosParallax = (float)(dt / (double)(dist1 * dist2));
          if (p[2] <= 0 && (double)cosParallax < 0.99998) go = false;
        }
        if (go) {
#pragma unroll
          for (int k = 0; k < 3; k++) p2[k] = (float)(dot3d(R[k * 3], R[k * 3 + 1], R[k * 3 + 2], p[0], p[1], p[2]) + (double)t[k]);
          if (p2[2] <= 0 && (double)cosParallax < 0.99998) go = false;
        }
        if (go) {
          const float invZ1 = 1.0f / p[2];
          const float im1x = P.fx * p[0] * invZ1 + P.cx, im1y = P.fy * p[1] * invZ1 + P.cy;
          const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
          if (squareError1 > th2) go = false;
        }
        if (go) {
          const float invZ2 = 1.0f / p2[2];
          const float im2x = P.fx * p2[0] * invZ2 + P.cx, im2y = P.fy * p2[1] * invZ2 + P.cy;
          const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
          if (squareError2 > th2) go = false;
        }
        if (go) {
          fl = (double)cosParallax < 0.99998 ? 3 : 1;
          cnt++;
          float* o = p3d + 3 * ((size_t)m * N + i);
          o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        }
      }
      sCos[i] = cosParallax; sCnt[i] = fl & 1;
      flags[(size_t)m * N + i] = fl;
    }
    sRed[tid] = cnt;
    if (tid == 0) sSel = 1.0f;
    __syncthreads();
    int nGood = 0;
    for (int k = 0; k < kRtThreads; k++) nGood += sRed[k];
    if (nGood > 0) {                     // sorted[min(50, size - 1)] by exact rank: ties are ordered by index
      const int want = min(50, nGood - 1);
      for (int i = tid; i < N; i += kRtThreads) {
        if (!sCnt[i]) continue;
        const float c = sCos[i];
        int rank = 0;
        for (int j = 0; j < N; j++) rank += (sCnt[j] && (sCos[j] < c || (sCos[j] == c && j < i))) ? 1 : 0;
        if (rank == want) sSel = c;
      }
    }
    __syncthreads();
    if (tid == 0) {
      rec->nGood[m] = nGood;
      rec->parallax[m] = nGood > 0 ? (float)((double)((float)acos((double)sSel) * 180.0f) / 3.1415926535897932384626433832795) : 0.f;
    }
  }

  if (!last_ticket(&tickets[1], kMotions, &sFlag)) return;
  if (tid == 0) {
    int chosen = -1;
    const int Nin = rec->n_inliers;
    const float minParallax = 1.0f;
    const int minTriangulated = 50;
    if (nm == 4) {                       // :504-574
      const int g0 = rec->nGood[0], g1 = rec->nGood[1], g2 = rec->nGood[2], g3 = rec->nGood[3];
      const int maxGood = max(g0, max(g1, max(g2, g3)));
      const int nMinGood = max((int)(0.9 * Nin), minTriangulated);
      int nsimilar = 0;
      if (g0 > 0.7 * maxGood) nsimilar++;
      if (g1 > 0.7 * maxGood) nsimilar++;
      if (g2 > 0.7 * maxGood) nsimilar++;
      if (g3 > 0.7 * maxGood) nsimilar++;
      if (!(maxGood < nMinGood || nsimilar > 1)) {
        if (maxGood == g0) { if (rec->parallax[0] > minParallax) chosen = 0; }
        else if (maxGood == g1) { if (rec->parallax[1] > minParallax) chosen = 1; }
        else if (maxGood == g2) { if (rec->parallax[2] > minParallax) chosen = 2; }
        else if (maxGood == g3) { if (rec->parallax[3] > minParallax) chosen = 3; }
      }
    } else if (nm == 8) {                // :693-735
      int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
      float bestParallax = -1.f;
      for (int i = 0; i < 8; i++) {
        const int nGood = rec->nGood[i];
        if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; bestSolutionIdx = i; bestParallax = rec->parallax[i]; }
        else if (nGood > secondBestGood) secondBestGood = nGood;
      }
      if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * Nin)
        chosen = bestSolutionIdx;
    }
    rec->best_motion = chosen;
    rec->success = chosen >= 0 ? 1 : 0;
    if (chosen >= 0) {
      for (int k = 0; k < 9; k++) rec->R21[k] = rec->R[chosen][k];
      for (int k = 0; k < 3; k++) rec->t21[k] = rec->t[chosen][k];
    }
    sChosen = chosen;
  }
  for (int i = tid; i < P.n1; i += kRtThreads) { outP3D[3 * (size_t)i] = 0.f; outP3D[3 * (size_t)i + 1] = 0.f; outP3D[3 * (size_t)i + 2] = 0.f; outTri[i] = 0; }
  __syncthreads();
  const int chosen = sChosen;
  if (chosen < 0) return;
  for (int i = tid; i < N; i += kRtThreads) {
    const uint8_t fl = flags[(size_t)chosen * N + i];
    if (!(fl & 1)) continue;
    const int k1 = idx1[i];
    const float* o = p3d + 3 * ((size_t)chosen * N + i);
    outP3D[3 * (size_t)k1] = o[0]; outP3D[3 * (size_t)k1 + 1] = o[1]; outP3D[3 * (size_t)k1 + 2] = o[2];
    if (fl & 2) outTri[k1] = 1;
  }
}

// ------------------------------------------------------------------------------------------------ host side

// Normalize, :753-799, over ALL keypoints of a frame: serial float sums in index order.  pn: n x 2, T: 3 x 3 row-major.
void normalize_keys(const float* keys, int n, float* pn, float* T) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) { meanX += keys[2 * i]; meanY += keys[2 * i + 1]; }
  meanX = meanX / n; meanY = meanY / n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    pn[2 * i] = keys[2 * i] - meanX; pn[2 * i + 1] = keys[2 * i + 1] - meanY;
    meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
  }
  meanDevX = meanDevX / n; meanDevY = meanDevY / n;
  const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
  for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
  for (int k = 0; k < 9; k++) T[k] = 0.f;
  T[0] = sX; T[4] = sY; T[8] = 1.f; T[2] = -meanX * sX; T[5] = -meanY * sY;
}

struct TvBufs {
  orbg::StageBlock blk;                // the one upload: 8 N floats, N keypoint indices, 8 H draws; the one download: TvRec, vP3D, vbTriangulated
  orbg::DevBuf<unsigned char> d_flags;
  orbg::DevBuf<float> d_hyp, d_scores, d_p3d;
  orbg::DevBuf<u64> d_masks;
  orbg::DevBuf<int> d_sets;
  orbg::DevBuf<unsigned> d_tickets;
  bool tickets_ready = false;
  std::vector<float> pn1, pn2, h_hyp;
  void release_buffers() {
    blk.release(); d_flags.release(); d_hyp.release(); d_scores.release();
    d_p3d.release(); d_masks.release(); d_sets.release(); d_tickets.release();
    tickets_ready = false;
  }
};
using TvWork = orbg::WorkArea<TvBufs>;
TvWork& tv_work() { static thread_local TvWork w; return w; }

int tv_check_draws(const int32_t* draws, int H, int n) {
  if (n < 8 || H < 0 || (H > 0 && !draws)) return ORBG_BAD_ARG;
  for (int k = 0; k < H; k++)
    for (int j = 0; j < 8; j++)
      if (draws[8 * (size_t)k + j] < 0 || draws[8 * (size_t)k + j] > n - 1 - j) return ORBG_BAD_ARG;
  return ORBG_OK;
}

}  // namespace

extern "C" int orbi_two_view_resolve_draws(int n, const int32_t* draws, int iterations, int32_t* idx) {
  if (n < 8 || iterations < 0 || (iterations > 0 && (!draws || !idx))) return ORBG_BAD_ARG;
  int rc = tv_check_draws(draws, iterations, n);
  if (rc) return rc;
  for (int k = 0; k < iterations; k++) {
    int r[8], o[8];
    for (int j = 0; j < 8; j++) r[j] = draws[8 * (size_t)k + j];
    orbg::resolve_draws<8>(n, r, o);
    for (int j = 0; j < 8; j++) idx[8 * (size_t)k + j] = o[j];
  }
  return ORBG_OK;
}

extern "C" int orbi_two_view_reconstruct(int device, const orbi_two_view_problem* p, const int32_t* draws, orbi_two_view_result* r) {
  if (!p || !r || p->struct_size < sizeof(orbi_two_view_problem) || r->struct_size < sizeof(orbi_two_view_result)) return ORBG_BAD_ARG;
  if (p->n1 < 0 || p->n2 < 0 || p->iterations < 1 || !draws) return ORBG_BAD_ARG;
  if ((p->n1 > 0 && (!p->keys1 || !p->matches12)) || (p->n2 > 0 && !p->keys2)) return ORBG_BAD_ARG;
  if (!(p->sigma > 0.f)) return ORBG_BAD_ARG;
  int N = 0;
  for (int i = 0; i < p->n1; i++) {
    if (p->matches12[i] >= p->n2) return ORBG_BAD_ARG;
    if (p->matches12[i] >= 0) N++;
  }
  if (N < 8) return ORBG_BAD_ARG;                     // no minimal set can be drawn
  const int H = p->iterations;
  if (N > ORBI_TWO_VIEW_MAX_MATCHES || H > ORBI_TWO_VIEW_MAX_ITERATIONS) return ORBG_CAP_EXCEEDED;
  int rc = tv_check_draws(draws, H, N);
  if (rc) return rc;
  TvWork& w = tv_work();
  if ((rc = w.open(device, "misc"))) return rc;
  hipStream_t st = w.stream;
  orbg::StreamDrain drain{st};

  TvParams P;
  memset(&P, 0, sizeof(P));
  P.N = N; P.n1 = p->n1; P.H = H; P.nG = (H + kGroup - 1) / kGroup; P.words = (N + 63) / 64;
  P.fx = p->fx; P.fy = p->fy; P.cx = p->cx; P.cy = p->cy; P.sigma = p->sigma;
  w.pn1.resize(2 * (size_t)std::max(p->n1, 1)); w.pn2.resize(2 * (size_t)std::max(p->n2, 1));
  normalize_keys(p->keys1, p->n1, w.pn1.data(), P.T1);
  normalize_keys(p->keys2, p->n2, w.pn2.data(), P.T2);
  inv3(P.T2, P.T2inv);

  orbg::StageBlock& S = w.blk;
  orbg::StageLayout lay;
  const auto s_f = lay.add<float>(8 * (size_t)N);            // in: one upload over the first three slots
  const auto s_idx1 = lay.add<int>(N);
  const auto s_draws = lay.add<int32_t>(8 * (size_t)H);
  const auto s_rec = lay.add<TvRec>(1);                      // out: one download over the last three
  const auto s_p3d = lay.add<float>(3 * (size_t)p->n1);
  const auto s_tri = lay.add<uint8_t>(p->n1);
  const size_t n_hyp = 2 * (size_t)H;
  if ((rc = S.reserve(lay.bytes())) || (rc = w.d_flags.reserve((size_t)kMotions * N)) || (rc = w.d_p3d.reserve(3 * (size_t)kMotions * N)) ||
      (rc = w.d_hyp.reserve(n_hyp * kHypFloats)) || (rc = w.d_scores.reserve(n_hyp)) || (rc = w.d_masks.reserve(n_hyp * P.words)) ||
      (rc = w.d_sets.reserve(8 * (size_t)H)))
    return rc;
  if (!w.tickets_ready) {                              // the tickets start at zero and every call leaves them at zero
    if ((rc = w.d_tickets.reserve(2))) return rc;
    ORBG_HIP(hipMemsetAsync(w.d_tickets.p, 0, w.d_tickets.cap * sizeof(unsigned), st));
    w.tickets_ready = true;
  }
  {
    float* f = S.host(s_f);
    int* k1 = S.host(s_idx1);
    int m = 0;
    for (int i = 0; i < p->n1; i++) {
      const int j = p->matches12[i];
      if (j < 0) continue;
      f[m] = p->keys1[2 * i]; f[(size_t)N + m] = p->keys1[2 * i + 1]; f[2 * (size_t)N + m] = p->keys2[2 * j]; f[3 * (size_t)N + m] = p->keys2[2 * j + 1];
      f[4 * (size_t)N + m] = w.pn1[2 * i]; f[5 * (size_t)N + m] = w.pn1[2 * i + 1]; f[6 * (size_t)N + m] = w.pn2[2 * j]; f[7 * (size_t)N + m] = w.pn2[2 * j + 1];
      k1[m] = i;
      m++;
    }
    S.put(s_draws, draws);
  }
  if ((rc = S.upload(s_f.off, s_draws.end(), st))) return rc;
  const float* d_f = S.device(s_f);
  const int* d_idx1 = S.device(s_idx1);
  const int* d_draws = S.device(s_draws);
  TvRec* d_rec = S.device(s_rec);
  float* d_P3D = S.device(s_p3d);
  uint8_t* d_tri = S.device(s_tri);
  hipLaunchKernelGGL(tv_ransac_kernel, dim3(2 * P.nG), dim3(kGroup), 0, st, P, d_f, d_draws, w.d_hyp.p, w.d_scores.p, w.d_masks.p,
                     w.d_sets.p, w.d_tickets.p, d_rec);
  ORBG_HIP(hipGetLastError());
  hipLaunchKernelGGL(tv_check_rt_kernel, dim3(kMotions), dim3(kRtThreads), 0, st, P, d_f, d_idx1, (const u64*)w.d_masks.p, d_rec,
                     (uint8_t*)w.d_flags.p, w.d_p3d.p, w.d_tickets.p, d_P3D, d_tri);
  ORBG_HIP(hipGetLastError());
  if ((rc = S.download(s_rec.off, s_tri.end(), st))) return rc;
  if (r->hyp_scores) ORBG_HIP(hipMemcpyAsync(r->hyp_scores, w.d_scores.p, n_hyp * 4, hipMemcpyDeviceToHost, st));
  if (r->hyp_masks) ORBG_HIP(hipMemcpyAsync(r->hyp_masks, w.d_masks.p, n_hyp * P.words * 8, hipMemcpyDeviceToHost, st));
  if (r->hyp_sets) ORBG_HIP(hipMemcpyAsync(r->hyp_sets, w.d_sets.p, 32 * (size_t)H, hipMemcpyDeviceToHost, st));
  if (r->hyp_models) {
    w.h_hyp.resize(n_hyp * kHypFloats);
    ORBG_HIP(hipMemcpyAsync(w.h_hyp.data(), w.d_hyp.p, n_hyp * kHypFloats * 4, hipMemcpyDeviceToHost, st));
  }
  ORBG_HIP(hipStreamSynchronize(st));
  if (r->hyp_models)
    for (size_t h = 0; h < n_hyp; h++) memcpy(r->hyp_models + 9 * h, w.h_hyp.data() + h * kHypFloats, 36);

  const TvRec& rec = *S.host(s_rec);
  r->success = rec.success; r->model = rec.model; r->best_iteration_H = rec.bestH; r->best_iteration_F = rec.bestF;
  r->n_matches = N; r->n_inliers = rec.n_inliers; r->n_motions = rec.n_motions; r->best_motion = rec.best_motion;
  r->h_degenerate = rec.h_degenerate; r->SH = rec.SH; r->SF = rec.SF;
  memcpy(r->H21, rec.H21, 36); memcpy(r->F21, rec.F21, 36); memcpy(r->R21, rec.R21, 36); memcpy(r->t21, rec.t21, 12);
  memcpy(r->T1, P.T1, 36); memcpy(r->T2, P.T2, 36);
  memcpy(r->motion_nGood, rec.nGood, sizeof(rec.nGood)); memcpy(r->motion_parallax, rec.parallax, sizeof(rec.parallax));
  memcpy(r->motion_R, rec.R, sizeof(rec.R)); memcpy(r->motion_t, rec.t, sizeof(rec.t));
  if (r->vP3D) S.get(s_p3d, r->vP3D);
  if (r->vbTriangulated) S.get(s_tri, r->vbTriangulated);
  return ORBG_OK;
}
