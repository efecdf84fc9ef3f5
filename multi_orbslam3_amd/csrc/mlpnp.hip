// MLPnPsolver (S/MLPnPsolver.cpp, I/MLPnPsolver.h) for gfx950: the RANSAC of Tracking::Relocalization.  Every hypothesis of a call -- and of
// every problem of a batch, the candidate keyframes of one Relocalization -- is evaluated in ONE kernel launch; the reference's serial loop
// (:99-216) is then replayed on the host over the per-hypothesis inlier counts in draw order.
//
// Grid = (hypotheses, problems); a workgroup is ONE wavefront and owns one hypothesis.  A hypothesis needs a 12 x 12 symmetric
// eigen-solve in FP64: a lane per hypothesis would hold about 300 doubles, so the wavefront shares the work and the matrices sit in LDS.
//   1  lanes 0..5: raw draws -> six indices (resolve_draws.hpp), point and bearing to double, a 2-D orthonormal null space of the bearing
//      by cross products (the reference takes it from an SVD; A^T A and the Gauss-Newton normal equations do not depend on the basis).
//   2  the planar test (:370-380): Eigen's FullPivHouseholderQR<Matrix3d> of points3 * points3^T restated, rank with the default
//      threshold epsilon * 3 relative to the largest pivot.  Planar: the eigen frame of that matrix (ascending eigenvalues, every
//      eigenvector signed so that its largest component is positive -- Eigen leaves the sign open).
//   3  A^T A (12 x 12, or 9 x 9 when planar) entry-wise over the lanes, every entry a sum over the 12 rows in row order.
//   4  cyclic Jacobi in the round-robin order: 11 steps per sweep, the 6 disjoint rotations of a step applied at once
//      (A' = J^T A J, V' = V J evaluated entry-wise from the old matrices, the lower triangle computed as its mirror entry so that A
//      stays exactly symmetric).  A sweep starts only while off^2 > 1e-30 * diag^2 (sums of squares), at most kMaxSweeps sweeps.  The
//      eigenvector of the smallest eigenvalue (the first on a tie) is result1 (:514-515; its sign is open there and here: what follows
//      does not depend on it).
//   5  :524-630 by every lane alike (wave-uniform values): the nearest rotation as the polar factor M (M^T M)^(-1/2) through a 3 x 3
//      Jacobi eigen-solve (equal to U V^T of the SVD for a regular M), the determinant fix, the scale, the two-way / four-way sign choice.
//      The inverse of [R | t] at :617 is taken as [R^T | -R^T t].
//   6  rot2rodrigues, mlpnp_gn (:687-752), rodrigues2rot.  Lane i builds the two Jacobian rows of point i from the closed form
//      N^T (I - v v^T) / |v| [ -R [X]x J_r(w) | I ] with J_r the right Jacobian of SO(3); the 6 x 6 normal equations entry-wise over the
//      lanes in row order, solved by an unpivoted LDL^T.  w = 0 gives 0 / 0 in J_r: a NaN pose, as the reference's generated Jacobian does.
//   7  CheckInliers (:255-286) wavefront-strided over the n correspondences: camera coordinates as double sums rounded to float, the
//      float projection of S/CameraModels/Pinhole.cpp:30-33, error2 < mvMaxError[i]; __ballot gives a mask word per step, popcount the count.
// Every reduction has a fixed order and there are no floating-point atomics: two runs give identical bits.
// Built with -ffp-contract=off and correctly rounded float divide / sqrt, like the rest of the library.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "resolve_draws.hpp"
#include "wave.hpp"

using orbg::select_device;

namespace {

constexpr int kThreads = 64;
constexpr int kMaxSweeps = 20;
constexpr double kSweepBound = 1e-30;

struct PnpDesc {                 // one problem of a launch
  int n, H, words, probe;        // probe: the six points in order, R0 / t0 instead of the linear stage (orbp_mlpnp_gn)
  long long off_pts;             // floats: X (3n), bearing (3n), P2D (2n), max_err (n)
  long long off_draws;           // int: 6 per hypothesis
  long long off_hyp;             // hypotheses before this problem's
  long long off_mask;            // 64-bit words before this problem's
  float k[4];                    // fx fy cx cy
  double R0[9], t0[3];
};

// ---- 3 x 3 helpers on registers (all indices are compile-time constants after unrolling)

template <int P, int Q>
__device__ __forceinline__ void rot3(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, h = t * apq;
  a[P][P] -= h; a[Q][Q] += h; a[P][Q] = 0.0; a[Q][P] = 0.0;
  constexpr int r = 3 - P - Q;
  const double arp = a[r][P], arq = a[r][Q];
  const double np = c * arp - s * arq, nq = s * arp + c * arq;
  a[r][P] = np; a[P][r] = np; a[r][Q] = nq; a[Q][r] = nq;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double vp = v[i][P], vq = v[i][Q];
    v[i][P] = c * vp - s * vq; v[i][Q] = s * vp + c * vq;
  }
}

// eigen-decomposition of the symmetric a: eigenvalues left on the diagonal, eigenvectors in the columns of v
__device__ __forceinline__ void sym3_eig(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    const double off2 = (a[0][1] * a[0][1] + a[0][2] * a[0][2]) + a[1][2] * a[1][2];
    const double diag2 = (a[0][0] * a[0][0] + a[1][1] * a[1][1]) + a[2][2] * a[2][2];
    if (!(off2 > 1e-32 * diag2)) break;
    rot3<0, 1>(a, v); rot3<0, 2>(a, v); rot3<1, 2>(a, v);
  }
}

__device__ __forceinline__ double det3(const double (&m)[3][3]) {
  return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

__device__ __forceinline__ void mul3(const double (&a)[3][3], const double (&b)[3][3], double (&c)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) c[i][j] = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j];
}

// U V^T of the SVD of m (the nearest rotation up to the determinant's sign) as the polar factor m (m^T m)^(-1/2)
__device__ __forceinline__ void polar3(const double (&m)[3][3], double (&r)[3][3]) {
  double s[3][3], w[3][3], q[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) s[i][j] = (m[0][i] * m[0][j] + m[1][i] * m[1][j]) + m[2][i] * m[2][j];
  sym3_eig(s, w);
  const double e0 = 1.0 / sqrt(s[0][0]), e1 = 1.0 / sqrt(s[1][1]), e2 = 1.0 / sqrt(s[2][2]);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) q[i][j] = (w[i][0] * e0 * w[j][0] + w[i][1] * e1 * w[j][1]) + w[i][2] * e2 * w[j][2];
  mul3(m, q, r);
}

// rodrigues2rot, :653-668
__device__ __forceinline__ void rodrigues2rot(const double (&w)[3], double (&R)[3][3]) {
  const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  double K2[3][3];
  mul3(K, K, K2);
  const bool on = th > DBL_EPSILON;
  const double a = sin(th) / th, b = (1.0 - cos(th)) / (th * th);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double I = i == j ? 1.0 : 0.0;
      R[i][j] = on ? (I + a * K[i][j]) + b * K2[i][j] : I;
    }
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// column c of the design matrix's row (point p, null vector nv), :429-503
__device__ __forceinline__ double design_entry(const double* p, const double* nv, int c, bool planar) {
  if (planar) return c < 6 ? nv[c >> 1] * p[1 + (c & 1)] : nv[c - 6];
  return c < 9 ? nv[c / 3] * p[c % 3] : nv[c - 9];
}

__global__ __launch_bounds__(kThreads) void mlpnp_ransac_kernel(const PnpDesc* __restrict__ descs, const float* __restrict__ pts,
                                                                const int* __restrict__ draws, double* __restrict__ poses,
                                                                int* __restrict__ counts, unsigned long long* __restrict__ masks) {
  const int b = blockIdx.y, h = blockIdx.x, lane = threadIdx.x;
  const PnpDesc& D = descs[b];
  const int n = D.n, H = D.H;
  if (h >= H) return;                                // a batch's grid is as wide as its longest problem (block-uniform)
  __shared__ double sP[6][3], sQ[6][3], sF[6][3], sN[6][2][3];   // points, points in the eigen frame, bearings, null spaces
  __shared__ double sA[12][12], sV[12][12];
  __shared__ double sAl[12], sBe[12];
  __shared__ int sPart[12];
  __shared__ double sJ[12][6], sRes[12], sNe[6][7], sDx[6];
  const float* X = pts + D.off_pts;
  const float* F = X + 3 * (size_t)n;
  const float* UV = F + 3 * (size_t)n;
  const float* ME = UV + 2 * (size_t)n;

  // ---- 1: the minimal set
  if (lane < 6) {
    int idx[6];
    if (D.probe) {
#pragma unroll
      for (int j = 0; j < 6; j++) idx[j] = j;
    } else {
      const int* dr = draws + D.off_draws + 6 * (size_t)h;
      const int r[6] = {dr[0], dr[1], dr[2], dr[3], dr[4], dr[5]};
      orbg::resolve_draws<6>(n, r, idx);
    }
    int me = idx[0];
#pragma unroll
    for (int j = 1; j < 6; j++) me = lane == j ? idx[j] : me;
    double f[3], e[3] = {0.0, 0.0, 0.0}, r[3], s[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { sP[lane][c] = (double)X[3 * (size_t)me + c]; f[c] = (double)F[3 * (size_t)me + c]; sF[lane][c] = f[c]; }
    // e: the axis of the bearing's smallest component (the first on a tie); r = f x e, s = f x r, both normalised
    const double a0 = fabs(f[0]), a1 = fabs(f[1]), a2 = fabs(f[2]);
    if (a0 <= a1 && a0 <= a2) e[0] = 1.0; else if (a1 <= a2) e[1] = 1.0; else e[2] = 1.0;
    cross3(f, e, r);
    const double nr = sqrt(dot3(r, r));
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = r[c] / nr;
    cross3(f, r, s);
    const double ns = sqrt(dot3(s, s));
#pragma unroll
    for (int c = 0; c < 3; c++) { sN[lane][0][c] = r[c]; sN[lane][1][c] = s[c] / ns; }
  }
  __syncthreads();

  // ---- 2: planar test and eigen frame (wave-uniform)
  bool planar = false;
  double eigenRot[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (!D.probe) {
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++) acc += sP[p][i] * sP[p][j];
        M[i][j] = acc;
      }
    // FullPivHouseholderQR<Matrix3d>::computeInPlace and rank()
    double q[3][3], piv[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) q[i][j] = M[i][j];
    const double prec = DBL_EPSILON * 3.0;
    double biggest = 0.0, maxpivot = 0.0;
    int nonzero = 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (nonzero < 3) continue;                     // finished early
      double big = -1.0;
      int br = k, bc = k;
#pragma unroll
      for (int j = k; j < 3; j++)                    // maxCoeff visits a column-major block column by column, the first maximum wins
#pragma unroll
        for (int i = k; i < 3; i++) {
          const double v = fabs(q[i][j]);
          if (v > big) { big = v; br = i; bc = j; }
        }
      if (k == 0) biggest = big;
      if (big <= biggest * prec) { nonzero = k; continue; }
#pragma unroll
      for (int i = k; i < 3; i++)
        if (br == i && i != k) {
#pragma unroll
          for (int j = 0; j < 3; j++) { const double t_ = q[k][j]; q[k][j] = q[i][j]; q[i][j] = t_; }
        }
#pragma unroll
      for (int j = k; j < 3; j++)
        if (bc == j && j != k) {
#pragma unroll
          for (int i = 0; i < 3; i++) { const double t_ = q[i][k]; q[i][k] = q[i][j]; q[i][j] = t_; }
        }
      // makeHouseholderInPlace on q[k..2][k]
      double tail2 = 0.0;
#pragma unroll
      for (int i = k + 1; i < 3; i++) tail2 += q[i][k] * q[i][k];
      const double c0 = q[k][k];
      double beta, tau, ess[3] = {0.0, 0.0, 0.0};
      if (tail2 <= DBL_MIN) { tau = 0.0; beta = c0; }
      else {
        beta = sqrt(c0 * c0 + tail2);
        if (c0 >= 0.0) beta = -beta;
#pragma unroll
        for (int i = k + 1; i < 3; i++) ess[i] = q[i][k] / (c0 - beta);
        tau = (beta - c0) / beta;
      }
      q[k][k] = beta;
      piv[k] = fabs(beta);
      if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
#pragma unroll
      for (int j = k + 1; j < 3; j++) {
        double wv = q[k][j];
#pragma unroll
        for (int i = k + 1; i < 3; i++) wv += ess[i] * q[i][j];
        q[k][j] -= tau * wv;
#pragma unroll
        for (int i = k + 1; i < 3; i++) q[i][j] -= tau * wv * ess[i];
      }
    }
    int rank = 0;
    const double thr = maxpivot * prec;
#pragma unroll
    for (int k = 0; k < 3; k++) rank += (k < nonzero && piv[k] > thr) ? 1 : 0;
    planar = rank == 2;
    if (planar) {
      double w[3][3];
      sym3_eig(M, w);
      double ev[3] = {M[0][0], M[1][1], M[2][2]};
      // ascending eigenvalues (stable), columns follow
#define ORBP_CSWAP(I, J)                                                                         \
  if (ev[J] < ev[I]) {                                                                           \
    const double t_ = ev[I]; ev[I] = ev[J]; ev[J] = t_;                                          \
    _Pragma("unroll") for (int r_ = 0; r_ < 3; r_++) { const double u_ = w[r_][I]; w[r_][I] = w[r_][J]; w[r_][J] = u_; } \
  }
      ORBP_CSWAP(0, 1) ORBP_CSWAP(1, 2) ORBP_CSWAP(0, 1)
#undef ORBP_CSWAP
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double a0 = fabs(w[0][j]), a1 = fabs(w[1][j]), a2 = fabs(w[2][j]);
        const double lead = (a0 >= a1 && a0 >= a2) ? w[0][j] : (a1 >= a2 ? w[1][j] : w[2][j]);
        const double sg = lead < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 3; i++) eigenRot[j][i] = sg * w[i][j];    // eigenvectors^T
      }
    }
  }
  if (lane < 6) {
#pragma unroll
    for (int i = 0; i < 3; i++) sQ[lane][i] = (eigenRot[i][0] * sP[lane][0] + eigenRot[i][1] * sP[lane][1]) + eigenRot[i][2] * sP[lane][2];
  }
  __syncthreads();

  double Rout[3][3], tout[3];
  if (D.probe) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) Rout[i][j] = D.R0[3 * i + j];
      tout[i] = D.t0[i];
    }
  } else {
    // ---- 3: A^T A
    const int nc = planar ? 9 : 12;
    for (int e = lane; e < 144; e += kThreads) {
      const int a = e / 12, c = e % 12;
      double acc = 0.0;
      if (a < nc && c < nc) {
        const int lo = min(a, c), hi = max(a, c);    // one order of the factors for both triangles: exactly symmetric
        for (int row = 0; row < 12; row++) {
          const double* p = planar ? sQ[row >> 1] : sP[row >> 1];
          const double* nv = sN[row >> 1][row & 1];
          acc += design_entry(p, nv, lo, planar) * design_entry(p, nv, hi, planar);
        }
      }
      sA[a][c] = acc;
      sV[a][c] = a == c ? 1.0 : 0.0;
    }
    __syncthreads();

    // ---- 4: parallel cyclic Jacobi
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
      double off2 = 0.0, diag2 = 0.0;
      for (int e = lane; e < 144; e += kThreads) {
        const int a = e / 12, c = e % 12;
        const double v = sA[a][c];
        if (a == c) diag2 += v * v; else if (a < c) off2 += v * v;
      }
      off2 = orbg::wave_sum_f64(off2);
      diag2 = orbg::wave_sum_f64(diag2);
      if (!(off2 > kSweepBound * diag2)) break;      // wave-uniform; also leaves on NaN
      for (int step = 0; step < 11; step++) {
        if (lane < 6) {
          int i0, i1;
          if (lane == 0) { i0 = 11; i1 = step; }
          else { i0 = (step + lane) % 11; i1 = (step + 11 - lane) % 11; }
          const int p = min(i0, i1), q = max(i0, i1);
          const double apq = sA[p][q];
          double c = 1.0, s = 0.0;
          if (apq != 0.0) {
            const double theta = (sA[q][q] - sA[p][p]) / (2.0 * apq);
            double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0.0) t = -t;
            c = 1.0 / sqrt(t * t + 1.0); s = t * c;
          }
          // column p of J is (c at p, -s at q), column q is (s at p, c at q)
          sAl[p] = c; sBe[p] = -s; sPart[p] = q;
          sAl[q] = c; sBe[q] = s; sPart[q] = p;
        }
        __syncthreads();
        double na[3], nv[3];
#pragma unroll
        for (int u = 0; u < 3; u++) {
          const int e = lane + u * kThreads;
          na[u] = 0.0; nv[u] = 0.0;
          if (e < 144) {
            const int r = e / 12, cidx = e % 12;
            const int i = min(r, cidx), j = max(r, cidx);
            const int ip = sPart[i], jp = sPart[j];
            const double ai = sAl[i], bi = sBe[i], aj = sAl[j], bj = sBe[j];
            na[u] = j == ip ? 0.0 : ai * (aj * sA[i][j] + bj * sA[i][jp]) + bi * (aj * sA[ip][j] + bj * sA[ip][jp]);
            const int cp = sPart[cidx];
            nv[u] = sAl[cidx] * sV[r][cidx] + sBe[cidx] * sV[r][cp];
          }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 3; u++) {
          const int e = lane + u * kThreads;
          if (e < 144) { sA[e / 12][e % 12] = na[u]; sV[e / 12][e % 12] = nv[u]; }
        }
        __syncthreads();
      }
    }
    int best = 0;
    double lam = sA[0][0];
    for (int k = 1; k < nc; k++)
      if (sA[k][k] < lam) { lam = sA[k][k]; best = k; }
    double x[12];
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = sV[k][best];

    // ---- 5: rotation, scale, sign (wave-uniform)
    if (planar) {
      double tmp0[3][3] = {{0.0, x[0], x[1]}, {0.0, x[2], x[3]}, {0.0, x[4], x[5]}};
      {
        const double c1[3] = {tmp0[0][1], tmp0[1][1], tmp0[2][1]}, c2[3] = {tmp0[0][2], tmp0[1][2], tmp0[2][2]};
        double c0[3];
        cross3(c1, c2, c0);
        tmp0[0][0] = c0[0]; tmp0[1][0] = c0[1]; tmp0[2][0] = c0[2];
      }
      double tmp[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) tmp[i][j] = tmp0[j][i];
      const double n1 = sqrt((tmp[0][1] * tmp[0][1] + tmp[1][1] * tmp[1][1]) + tmp[2][1] * tmp[2][1]);
      const double n2 = sqrt((tmp[0][2] * tmp[0][2] + tmp[1][2] * tmp[1][2]) + tmp[2][2] * tmp[2][2]);
      const double scale = 1.0 / sqrt(fabs(n1 * n2));
      double R1[3][3], R1e[3][3];
      polar3(tmp, R1);
      if (det3(R1) < 0.0) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) R1[i][j] = R1[i][j] * -1.0;
      }
      double eT[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) eT[i][j] = eigenRot[j][i];
      mul3(eT, R1, R1e);
      const double t[3] = {scale * x[6], scale * x[7], scale * x[8]};
      double Ra[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Ra[i][j] = R1e[j][i] * -1.0;
      if (det3(Ra) < 0.0) {
#pragma unroll
        for (int i = 0; i < 3; i++) Ra[i][2] = Ra[i][2] * -1.0;
      }
      double bestn = 0.0;
      int bi = 0;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const double sr = c < 2 ? 1.0 : -1.0, st = (c & 1) ? -1.0 : 1.0;
        double norms = 0.0;
        for (int p = 0; p < 6; p++) {
          double v[3];
#pragma unroll
          for (int i = 0; i < 3; i++) v[i] = ((sr * Ra[i][0] * sP[p][0] + sr * Ra[i][1] * sP[p][1]) + Ra[i][2] * sP[p][2]) + st * t[i];
          const double nv_ = sqrt(dot3(v, v));
          norms += 1.0 - ((v[0] / nv_ * sF[p][0] + v[1] / nv_ * sF[p][1]) + v[2] / nv_ * sF[p][2]);
        }
        if (c == 0 || norms < bestn) { bestn = norms; bi = c; }     // std::min_element: the first minimum
      }
      const double sr = bi < 2 ? 1.0 : -1.0, st = (bi & 1) ? -1.0 : 1.0;
#pragma unroll
      for (int i = 0; i < 3; i++) { Rout[i][0] = sr * Ra[i][0]; Rout[i][1] = sr * Ra[i][1]; Rout[i][2] = Ra[i][2]; tout[i] = st * t[i]; }
    } else {
      double tmp[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) tmp[i][j] = x[3 * j + i];
      double cn[3];
#pragma unroll
      for (int j = 0; j < 3; j++) cn[j] = sqrt((tmp[0][j] * tmp[0][j] + tmp[1][j] * tmp[1][j]) + tmp[2][j] * tmp[2][j]);
      const double scale = 1.0 / pow(fabs(cn[0] * cn[1] * cn[2]), 1.0 / 3.0);
      double R[3][3];
      polar3(tmp, R);
      if (det3(R) < 0.0) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) R[i][j] = R[i][j] * -1.0;
      }
      const double ts[3] = {scale * x[9], scale * x[10], scale * x[11]};
      double t1[3], ti[3];
#pragma unroll
      for (int i = 0; i < 3; i++) t1[i] = (R[i][0] * ts[0] + R[i][1] * ts[1]) + R[i][2] * ts[2];
      // Ts[s] = [R | +-tout]^-1 = [R^T | -+ R^T tout]
#pragma unroll
      for (int i = 0; i < 3; i++) ti[i] = -((R[0][i] * t1[0] + R[1][i] * t1[1]) + R[2][i] * t1[2]);
      double err[2] = {0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const double sg = s == 0 ? 1.0 : -1.0;
        for (int p = 0; p < 6; p++) {
          double v[3];
#pragma unroll
          for (int i = 0; i < 3; i++) v[i] = ((R[0][i] * sP[p][0] + R[1][i] * sP[p][1]) + R[2][i] * sP[p][2]) + sg * ti[i];
          const double nv_ = sqrt(dot3(v, v));
          err[s] += 1.0 - ((v[0] / nv_ * sF[p][0] + v[1] / nv_ * sF[p][1]) + v[2] / nv_ * sF[p][2]);
        }
      }
      const double sg = err[0] < err[1] ? 1.0 : -1.0;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        tout[i] = sg * ti[i];
#pragma unroll
        for (int j = 0; j < 3; j++) Rout[i][j] = R[j][i];
      }
    }
  }

  // ---- 6: Gauss-Newton on (rodrigues, t)
  double xw[3] = {0.0, 0.0, 0.0}, xt[3] = {tout[0], tout[1], tout[2]};
  {
    const double trace = ((Rout[0][0] + Rout[1][1]) + Rout[2][2]) - 1.0;
    const double wn = acos(trace / 2.0);
    if (wn > DBL_EPSILON) {
      const double sc = wn / (2.0 * sin(wn));
      xw[0] = (Rout[2][1] - Rout[1][2]) * sc; xw[1] = (Rout[0][2] - Rout[2][0]) * sc; xw[2] = (Rout[1][0] - Rout[0][1]) * sc;
    }
  }
  for (int it = 0; it < 5; it++) {
    double R[3][3];
    rodrigues2rot(xw, R);
    const double th2 = (xw[0] * xw[0] + xw[1] * xw[1]) + xw[2] * xw[2], th = sqrt(th2);
    const double ja = (1.0 - cos(th)) / th2, jb = (th - sin(th)) / (th2 * th);      // J_r = I - ja [w]x + jb [w]x^2; 0 / 0 at w = 0
    if (lane < 6) {
      double v[3];
#pragma unroll
      for (int i = 0; i < 3; i++) v[i] = ((R[i][0] * sP[lane][0] + R[i][1] * sP[lane][1]) + R[i][2] * sP[lane][2]) + xt[i];
      const double nv_ = sqrt(dot3(v, v));
      const double vh[3] = {v[0] / nv_, v[1] / nv_, v[2] / nv_};
      const double Xp[3] = {sP[lane][0], sP[lane][1], sP[lane][2]};
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const double nk[3] = {sN[lane][k][0], sN[lane][k][1], sN[lane][k][2]};
        const double d = dot3(nk, vh);
        sRes[2 * lane + k] = d;
        const double g[3] = {(nk[0] - vh[0] * d) / nv_, (nk[1] - vh[1] * d) / nv_, (nk[2] - vh[2] * d) / nv_};
        double u[3], w[3], c1[3], c2[3];
#pragma unroll
        for (int i = 0; i < 3; i++) u[i] = (R[0][i] * g[0] + R[1][i] * g[1]) + R[2][i] * g[2];
        cross3(u, Xp, w);
        cross3(xw, w, c1);
        cross3(xw, c1, c2);
#pragma unroll
        for (int i = 0; i < 3; i++) { sJ[2 * lane + k][i] = -((w[i] + ja * c1[i]) + jb * c2[i]); sJ[2 * lane + k][3 + i] = g[i]; }
      }
    }
    __syncthreads();
    if (lane < 42) {
      const int a = lane / 7, c = lane % 7;
      double acc = 0.0;
      for (int row = 0; row < 12; row++) acc += sJ[row][a] * (c < 6 ? sJ[row][c] : sRes[row]);
      sNe[a][c] = acc;
    }
    __syncthreads();
    if (lane == 0) {
      // LDL^T in place (L below the diagonal, d on it), then the two triangular solves
      for (int j = 0; j < 6; j++) {
        double dj = sNe[j][j];
        for (int k = 0; k < j; k++) dj -= sNe[j][k] * sNe[j][k] * sNe[k][k];
        sNe[j][j] = dj;
        for (int i = j + 1; i < 6; i++) {
          double l = sNe[i][j];
          for (int k = 0; k < j; k++) l -= sNe[i][k] * sNe[j][k] * sNe[k][k];
          sNe[i][j] = l / dj;
        }
      }
      for (int i = 0; i < 6; i++) {
        double acc = sNe[i][6];
        for (int k = 0; k < i; k++) acc -= sNe[i][k] * sDx[k];
        sDx[i] = acc;
      }
      for (int i = 0; i < 6; i++) sDx[i] = sDx[i] / sNe[i][i];
      for (int i = 5; i >= 0; i--) {
        double acc = sDx[i];
        for (int k = i + 1; k < 6; k++) acc -= sNe[k][i] * sDx[k];
        sDx[i] = acc;
      }
    }
    __syncthreads();
    double dx[6];
    bool any_big = false, all_gt1 = true;
#pragma unroll
    for (int i = 0; i < 6; i++) { dx[i] = sDx[i]; any_big = any_big || fabs(dx[i]) > 5.0; all_gt1 = all_gt1 && fabs(dx[i]) > 1.0; }
    bool small = true;
    for (int row = 0; row < 12; row++) {
      double dl = 0.0;
#pragma unroll
      for (int i = 0; i < 6; i++) dl += sJ[row][i] * dx[i];
      small = small && fabs(dl) < 1e-5;
    }
    __syncthreads();                                 // sJ / sDx are rewritten by the next iteration
    if (any_big || all_gt1) break;                   // :738: the step is not applied
#pragma unroll
    for (int i = 0; i < 3; i++) { xw[i] = xw[i] - dx[i]; xt[i] = xt[i] - dx[3 + i]; }
    if (small) break;
  }
  double R[3][3];
  rodrigues2rot(xw, R);
  if (lane == 0) {
    double* o = poses + 12 * (size_t)(D.off_hyp + h);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) o[3 * i + j] = R[i][j];
      o[9 + i] = xt[i];
    }
  }

  // ---- 7: CheckInliers
  int cnt = 0;
  unsigned long long* mrow = masks + D.off_mask + (size_t)h * D.words;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool ok = false;
    if (i < n) {
      const float px = X[3 * (size_t)i], py = X[3 * (size_t)i + 1], pz = X[3 * (size_t)i + 2];
      const float xc = (float)((((R[0][0] * (double)px + R[0][1] * (double)py) + R[0][2] * (double)pz)) + xt[0]);
      const float yc = (float)((((R[1][0] * (double)px + R[1][1] * (double)py) + R[1][2] * (double)pz)) + xt[1]);
      const float zc = (float)((((R[2][0] * (double)px + R[2][1] * (double)py) + R[2][2] * (double)pz)) + xt[2]);
      const float u = D.k[0] * xc / zc + D.k[2], v = D.k[1] * yc / zc + D.k[3];
      const float dX = UV[2 * (size_t)i] - u, dY = UV[2 * (size_t)i + 1] - v;
      const float e2 = dX * dX + dY * dY;
      ok = e2 < ME[i];                               // a NaN error compares false: outlier
    }
    const unsigned long long bal = __ballot(ok);
    cnt += __popcll(bal);
    if (lane == 0) mrow[i0 >> 6] = bal;              // one writer per word
  }
  if (lane == 0) { counts[2 * (D.off_hyp + h)] = cnt; counts[2 * (D.off_hyp + h) + 1] = planar ? 1 : 0; }
}

// ------------------------------------------------------------------------------------------------ host side

struct PnpRansac { int min_inliers, max_its; float epsilon; };

// SetRansacParameters, S/MLPnPsolver.cpp:218-248, in the reference's types
PnpRansac ransac_parameters(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon) {
  int nMinInliers = (int)((float)N * epsilon);
  if (nMinInliers < min_inliers) nMinInliers = min_inliers;
  if (nMinInliers < min_set) nMinInliers = min_set;
  if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
  int nIterations;
  if (nMinInliers == N) nIterations = 1;
  else {
    const double v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3)));
    // ceil() of a NaN / an infinity converted to int is INT_MIN with the x86 conversion the reference is built for: pinned here
    nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
  }
  return PnpRansac{nMinInliers, std::max(1, std::min(nIterations, max_iterations)), epsilon};
}

struct PnpBufs {
  orbg::StageBlock blk;            // problems and draws up, hypotheses down
  orbg::StreamSignal sig;
  void release_buffers() { blk.release(); sig.release(); }
};
using PnpWork = orbg::WorkArea<PnpBufs>;

struct PnpJob {                  // one problem of a launch, host view
  const orbp_mlpnp_problem* p;
  const float* max_err;          // n
  int H, probe;
  const int32_t* draws;
  const double* R0; const double* t0;
};

struct PnpOut {                  // where a launch's outputs are on the host
  const double* poses; const unsigned long long* masks; const int* counts;
  std::vector<PnpDesc> desc;
};

int check_problem(const orbp_mlpnp_problem* p) {
  if (!p || p->struct_size < sizeof(orbp_mlpnp_problem) || p->n < 0 || p->m < 0) return ORBG_BAD_ARG;
  if (p->n > 0 && (!p->P2D || !p->sigma2 || !p->bearing || !p->P3Dw || !p->kp_index)) return ORBG_BAD_ARG;
  if (p->camera.model != ORBG_CAM_PINHOLE) return ORBG_BAD_ARG;     // nothing else is approximated
  for (int i = 0; i < p->n; i++)
    if (p->kp_index[i] < 0 || p->kp_index[i] >= p->m) return ORBG_BAD_ARG;
  return ORBG_OK;
}

// raw RandomInt results: draw j of an iteration picks from a list of n - j entries (:128)
int check_draws(const int32_t* draws, int H, int n) {
  if (H > 0 && (!draws || n < 6)) return ORBG_BAD_ARG;
  for (int k = 0; k < H; k++)
    for (int j = 0; j < 6; j++)
      if (draws[6 * (size_t)k + j] < 0 || draws[6 * (size_t)k + j] > n - 1 - j) return ORBG_BAD_ARG;
  return ORBG_OK;
}

// One upload, one launch over `jobs` (each with H >= 1, n >= 6, checked), one download, one wait on the sequence word.
int launch(PnpWork& w, const std::vector<PnpJob>& jobs, PnpOut& out) {
  const int B = (int)jobs.size();
  hipStream_t st = w.stream;
  out.desc.resize(B);
  long long o_pts = 0, o_draws = 0, o_hyp = 0, o_mask = 0;
  int max_h = 0;
  for (int b = 0; b < B; b++) {
    const PnpJob& j = jobs[b];
    PnpDesc& D = out.desc[b];
    memset(&D, 0, sizeof(D));
    D.n = j.p->n; D.H = j.H; D.words = (D.n + 63) / 64; D.probe = j.probe;
    D.off_pts = o_pts; D.off_draws = o_draws; D.off_hyp = o_hyp; D.off_mask = o_mask;
    D.k[0] = j.p->camera.fx; D.k[1] = j.p->camera.fy; D.k[2] = j.p->camera.cx; D.k[3] = j.p->camera.cy;
    if (j.probe) { memcpy(D.R0, j.R0, sizeof(D.R0)); memcpy(D.t0, j.t0, sizeof(D.t0)); }
    o_pts += 9LL * D.n; o_draws += 6LL * j.H; o_hyp += j.H; o_mask += (long long)j.H * D.words;
    max_h = std::max(max_h, j.H);
  }
  orbg::StageBlock& S = w.blk;
  orbg::StageLayout lay;
  const auto s_desc = lay.add<PnpDesc>(B);                              // in: one upload over the first three slots
  const auto s_pts = lay.add<float>((size_t)o_pts);
  const auto s_draws = lay.add<int32_t>((size_t)o_draws);
  const auto s_pose = lay.add<double>(12 * (size_t)o_hyp);              // out: one download over the last three
  const auto s_mask = lay.add<unsigned long long>((size_t)o_mask);
  const auto s_cnt = lay.add<int>(2 * (size_t)o_hyp);
  int rc;
  if ((rc = S.reserve(lay.bytes()))) return rc;
  S.put(s_desc, out.desc.data());
  float* hf = S.host(s_pts);
  int32_t* hd = S.host(s_draws);
  for (int b = 0; b < B; b++) {
    const PnpJob& j = jobs[b];
    const PnpDesc& D = out.desc[b];
    const size_t n = D.n;
    float* f = hf + D.off_pts;
    memcpy(f, j.p->P3Dw, 12 * n); memcpy(f + 3 * n, j.p->bearing, 12 * n); memcpy(f + 6 * n, j.p->P2D, 8 * n); memcpy(f + 8 * n, j.max_err, 4 * n);
    if (j.probe) memset(hd + D.off_draws, 0, 24 * (size_t)j.H);
    else memcpy(hd + D.off_draws, j.draws, 24 * (size_t)j.H);
  }
  if ((rc = S.upload(s_desc.off, s_draws.end(), st))) return rc;
  hipLaunchKernelGGL(mlpnp_ransac_kernel, dim3(max_h, B), dim3(kThreads), 0, st, (const PnpDesc*)S.device(s_desc), (const float*)S.device(s_pts),
                     (const int*)S.device(s_draws), S.device(s_pose), S.device(s_cnt), S.device(s_mask));
  ORBG_HIP(hipGetLastError());
  if ((rc = S.download(s_pose.off, s_cnt.end(), st)) || (rc = w.sig.sync(st))) return rc;
  out.poses = S.host(s_pose); out.masks = S.host(s_mask); out.counts = S.host(s_cnt);
  return ORBG_OK;
}

}  // namespace

// The state MLPnPsolver keeps between iterate() calls (I/MLPnPsolver.h) plus the flat problem
struct orbp_mlpnp {
  PnpWork w;
  bool have_problem = false;
  orbp_mlpnp_problem prob;
  std::vector<float> P2D, sigma2, bearing, P3Dw, max_err;
  std::vector<int32_t> kp_index;
  int min_inliers = 8, max_its = 300;                 // mRansacMinInliers, mRansacMaxIts
  int iterations = 0, best_inliers = 0;               // mnIterations, mnBestInliers
  int best_iteration = -1;
  bool have_best = false;
  float best_Tcw[16];                                 // mBestTcw
  std::vector<uint8_t> best_mask;                     // mvbBestInliers (n)
};

namespace {

void pose_to_Tcw(const double* pose, float* T) {      // Rcw / tcw .convertTo(CV_32F) into eye(4, 4), :175-181
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = (float)pose[3 * i + j];
    T[4 * i + 3] = (float)pose[9 + i];
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

void clear_result(orbp_mlpnp_result* r, int m) {
  r->no_more = 0; r->returned = 0; r->n_inliers = 0; r->iterations_done = 0; r->iterations_run = 0; r->best_iteration = -1;
  r->have_best = 0; r->best_inliers = 0;
  memset(r->Tcw, 0, sizeof(r->Tcw)); memset(r->best_Tcw, 0, sizeof(r->best_Tcw));
  if (r->inliers && m > 0) memset(r->inliers, 0, m);
}

void copy_hyp(const PnpOut& o, int b, orbp_mlpnp_result* r) {
  const PnpDesc& D = o.desc[b];
  for (int h = 0; h < D.H; h++) {
    if (r->hyp_n_inliers) r->hyp_n_inliers[h] = o.counts[2 * (D.off_hyp + h)];
    if (r->hyp_planar) r->hyp_planar[h] = o.counts[2 * (D.off_hyp + h) + 1];
    if (r->hyp_R) memcpy(r->hyp_R + 9 * (size_t)h, o.poses + 12 * (size_t)(D.off_hyp + h), 72);
    if (r->hyp_t) memcpy(r->hyp_t + 3 * (size_t)h, o.poses + 12 * (size_t)(D.off_hyp + h) + 9, 24);
  }
  if (r->hyp_masks) memcpy(r->hyp_masks, o.masks + D.off_mask, 8 * (size_t)D.H * D.words);
}

// the state of one solver across the replay
struct PnpState {
  int min_inliers, max_its, iterations, best_inliers, best_iteration;
  bool have_best;
  float* best_Tcw;               // 16
  uint8_t* best_mask;            // n
};

// The loop of :113-215 over the counts of hypotheses 0 .. H-1 of job b in draw order, with Refine() as it behaves (:288-342): it
// returns the CURRENT hypothesis, and exactly when its count exceeds min_inliers.
void replay(const PnpOut& o, int b, const orbp_mlpnp_problem* p, PnpState& s, orbp_mlpnp_result* r) {
  const PnpDesc& D = o.desc[b];
  const int n = D.n;
  int ret = -1, run = 0;
  for (int h = 0; h < D.H; h++) {
    run++; s.iterations++;
    const int c = o.counts[2 * (D.off_hyp + h)];
    if (c >= s.min_inliers) {
      if (c > s.best_inliers) {
        s.best_inliers = c; s.have_best = true; s.best_iteration = s.iterations - 1;
        pose_to_Tcw(o.poses + 12 * (size_t)(D.off_hyp + h), s.best_Tcw);
        const unsigned long long* mw = o.masks + D.off_mask + (size_t)h * D.words;
        for (int i = 0; i < n; i++) s.best_mask[i] = (uint8_t)((mw[i >> 6] >> (i & 63)) & 1ULL);
      }
      if (c > s.min_inliers) { ret = h; break; }
    }
  }
  r->iterations_run = run;
  if (ret >= 0) {
    r->returned = 1; r->n_inliers = o.counts[2 * (D.off_hyp + ret)];
    pose_to_Tcw(o.poses + 12 * (size_t)(D.off_hyp + ret), r->Tcw);
    if (r->inliers) {
      const unsigned long long* mw = o.masks + D.off_mask + (size_t)ret * D.words;
      for (int i = 0; i < n; i++)
        if ((mw[i >> 6] >> (i & 63)) & 1ULL) r->inliers[p->kp_index[i]] = 1;
    }
  } else if (s.iterations >= s.max_its) {
    r->no_more = 1;
    if (s.best_inliers >= s.min_inliers) {
      r->returned = 1; r->n_inliers = s.best_inliers;
      memcpy(r->Tcw, s.best_Tcw, 64);
      if (r->inliers)
        for (int i = 0; i < n; i++)
          if (s.best_mask[i]) r->inliers[p->kp_index[i]] = 1;
    }
  }
}

void finish_result(const PnpState& s, orbp_mlpnp_result* r) {
  r->iterations_done = s.iterations; r->have_best = s.have_best ? 1 : 0; r->best_inliers = s.best_inliers;
  r->best_iteration = s.best_iteration;
  if (s.have_best) memcpy(r->best_Tcw, s.best_Tcw, 64);
}

void max_errors(const float* sigma2, int n, float th2, float* out) {
  for (int i = 0; i < n; i++) out[i] = sigma2[i] * th2;               // :250-252, float
}

PnpWork& batch_work() { static thread_local PnpWork w; return w; }

}  // namespace

extern "C" int orbp_mlpnp_ransac_iterations(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                            int* max_its, int* min_inliers_out) {
  if (n < 0 || min_set != 6 || (!max_its && !min_inliers_out)) return ORBG_BAD_ARG;
  const PnpRansac q = ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon);
  if (max_its) *max_its = q.max_its;
  if (min_inliers_out) *min_inliers_out = q.min_inliers;
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_resolve_draws(int n, const int32_t* draws, int n_iterations, int32_t* idx) {
  if (n < 6 || n_iterations < 0 || (n_iterations > 0 && (!draws || !idx))) return ORBG_BAD_ARG;
  int rc = check_draws(draws, n_iterations, n);
  if (rc) return rc;
  for (int k = 0; k < n_iterations; k++) {
    int r[6], o[6];
    for (int j = 0; j < 6; j++) r[j] = draws[6 * (size_t)k + j];
    orbg::resolve_draws<6>(n, r, o);
    for (int j = 0; j < 6; j++) idx[6 * (size_t)k + j] = o[j];
  }
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_create(int device, orbp_mlpnp** out) {
  if (!out) return ORBG_BAD_ARG;
  int rc = select_device(device);
  if (rc) return rc;
  orbp_mlpnp* h = new orbp_mlpnp;
  if ((rc = h->w.open(device, "misc"))) { delete h; return rc; }
  *out = h;
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_destroy(orbp_mlpnp* h) {
  if (!h) return ORBG_OK;
  h->w.release();
  delete h;
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_set_stream(orbp_mlpnp* h, void* hip_stream) {
  if (!h) return ORBG_BAD_ARG;
  int rc = select_device(h->w.device);
  if (rc) return rc;
  return orbg::swap_stream(&h->w.stream, &h->w.ext_stream, hip_stream, "misc");
}

extern "C" int orbp_mlpnp_set_problem(orbp_mlpnp* h, const orbp_mlpnp_problem* p) {
  if (!h) return ORBG_BAD_ARG;
  int rc = check_problem(p);
  if (rc) return rc;
  const size_t n = p->n;
  h->P2D.assign(p->P2D, p->P2D + 2 * n); h->sigma2.assign(p->sigma2, p->sigma2 + n); h->bearing.assign(p->bearing, p->bearing + 3 * n);
  h->P3Dw.assign(p->P3Dw, p->P3Dw + 3 * n); h->kp_index.assign(p->kp_index, p->kp_index + n);
  memset(&h->prob, 0, sizeof(h->prob));
  memcpy(&h->prob, p, sizeof(orbp_mlpnp_problem));
  h->prob.P2D = h->P2D.data(); h->prob.sigma2 = h->sigma2.data(); h->prob.bearing = h->bearing.data(); h->prob.P3Dw = h->P3Dw.data();
  h->prob.kp_index = h->kp_index.data();
  h->have_problem = true;
  h->iterations = 0; h->best_inliers = 0; h->best_iteration = -1; h->have_best = false;
  h->best_mask.assign(n, 0);
  h->max_err.resize(n);
  // the constructor ends with SetRansacParameters() at its defaults, :95, I/MLPnPsolver.h
  const PnpRansac q = ransac_parameters((int)n, 0.99, 8, 300, 6, 0.4f);
  h->min_inliers = q.min_inliers; h->max_its = q.max_its;
  max_errors(h->sigma2.data(), (int)n, 5.991f, h->max_err.data());
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_set_ransac_parameters(orbp_mlpnp* h, double probability, int min_inliers, int max_iterations, int min_set,
                                                float epsilon, float th2) {
  if (!h || !h->have_problem || min_set != 6) return ORBG_BAD_ARG;
  const PnpRansac q = ransac_parameters(h->prob.n, probability, min_inliers, max_iterations, min_set, epsilon);
  h->min_inliers = q.min_inliers; h->max_its = q.max_its;             // mnIterations and the best so far are NOT reset (:218-253)
  max_errors(h->sigma2.data(), h->prob.n, th2, h->max_err.data());
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_iterations_of_call(orbp_mlpnp* h, int n_iterations, int* k) {
  if (!h || !h->have_problem || !k || n_iterations < 0) return ORBG_BAD_ARG;
  // :104 and the OR of :113
  *k = h->prob.n < h->min_inliers ? 0 : std::max(n_iterations, h->max_its - h->iterations);
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_iterate(orbp_mlpnp* h, int n_iterations, const int32_t* draws, orbp_mlpnp_result* r) {
  if (!h || !h->have_problem || !r || r->struct_size < sizeof(orbp_mlpnp_result) || n_iterations < 0) return ORBG_BAD_ARG;
  const int n = h->prob.n;
  if (n < h->min_inliers) {                                             // :104-108, no launch
    clear_result(r, h->prob.m);
    r->no_more = 1; r->iterations_done = h->iterations; r->have_best = h->have_best ? 1 : 0; r->best_inliers = h->best_inliers;
    r->best_iteration = h->best_iteration;
    if (h->have_best) memcpy(r->best_Tcw, h->best_Tcw, 64);
    return ORBG_OK;
  }
  const int H = std::max(n_iterations, h->max_its - h->iterations);
  int rc = check_draws(draws, H, n);
  if (rc) return rc;
  PnpState s{h->min_inliers, h->max_its, h->iterations, h->best_inliers, h->best_iteration, h->have_best, h->best_Tcw, h->best_mask.data()};
  if (H > 0) {
    if ((rc = select_device(h->w.device))) return rc;
    std::vector<PnpJob> jobs(1);
    jobs[0] = PnpJob{&h->prob, h->max_err.data(), H, 0, draws, nullptr, nullptr};
    PnpOut o;
    if ((rc = launch(h->w, jobs, o))) return rc;
    clear_result(r, h->prob.m);
    copy_hyp(o, 0, r);
    replay(o, 0, &h->prob, s, r);
  } else {
    clear_result(r, h->prob.m);
    if (s.iterations >= s.max_its) {
      r->no_more = 1;
      if (s.best_inliers >= s.min_inliers) {
        r->returned = 1; r->n_inliers = s.best_inliers; memcpy(r->Tcw, s.best_Tcw, 64);
        if (r->inliers)
          for (int i = 0; i < n; i++)
            if (s.best_mask[i]) r->inliers[h->prob.kp_index[i]] = 1;
      }
    }
  }
  h->iterations = s.iterations; h->best_inliers = s.best_inliers; h->best_iteration = s.best_iteration; h->have_best = s.have_best;
  finish_result(s, r);
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_solve_batch(int device, const orbp_mlpnp_problem* problems, int B, const orbp_mlpnp_params* params,
                                      const int32_t* const* draws, orbp_mlpnp_result* results) {
  if (B < 0 || (B > 0 && (!problems || !params || !draws || !results))) return ORBG_BAD_ARG;
  // every argument is checked, and the device, before any result is written: a call that fails leaves `results` as it found them
  std::vector<PnpJob> jobs;
  std::vector<int> job_of(B, -1);
  std::vector<PnpRansac> q(B);
  std::vector<std::vector<float>> me(B);
  int rc;
  for (int b = 0; b < B; b++) {
    if ((rc = check_problem(&problems[b]))) return rc;
    if (results[b].struct_size < sizeof(orbp_mlpnp_result) || params[b].min_set != 6) return ORBG_BAD_ARG;
    const int n = problems[b].n;
    q[b] = ransac_parameters(n, params[b].probability, params[b].min_inliers, params[b].max_iterations, 6, params[b].epsilon);
    if (n < q[b].min_inliers) continue;                           // :104-108: bNoMore, no launch
    if ((rc = check_draws(draws[b], q[b].max_its, n))) return rc;
    me[b].resize(n);
    max_errors(problems[b].sigma2, n, params[b].th2, me[b].data());
    job_of[b] = (int)jobs.size();
    jobs.push_back(PnpJob{&problems[b], me[b].data(), q[b].max_its, 0, draws[b], nullptr, nullptr});
  }
  rc = select_device(device);
  if (rc) return rc;
  PnpOut o;
  if (!jobs.empty()) {
    PnpWork& w = batch_work();
    if ((rc = w.open(device, "misc"))) return rc;
    if ((rc = launch(w, jobs, o))) return rc;
  }
  for (int b = 0; b < B; b++) {
    orbp_mlpnp_result* r = &results[b];
    clear_result(r, problems[b].m);
    if (job_of[b] < 0) { r->no_more = 1; continue; }
    const int n = problems[b].n;
    float best_T[16];
    std::vector<uint8_t> best_mask(n, 0);
    PnpState s{q[b].min_inliers, q[b].max_its, 0, 0, -1, false, best_T, best_mask.data()};
    copy_hyp(o, job_of[b], r);
    replay(o, job_of[b], &problems[b], s, r);
    finish_result(s, r);
  }
  return ORBG_OK;
}

extern "C" int orbp_mlpnp_gn(int device, const float* P3Dw, const float* bearing, const double* R, const double* t, double* R_out,
                             double* t_out) {
  if (!P3Dw || !bearing || !R || !t || !R_out || !t_out) return ORBG_BAD_ARG;
  int rc = select_device(device);
  if (rc) return rc;
  const float zeros[12] = {0};
  const int32_t kp[6] = {0, 1, 2, 3, 4, 5};
  orbp_mlpnp_problem p;
  memset(&p, 0, sizeof(p));
  p.struct_size = sizeof(p); p.n = 6; p.m = 6; p.P2D = zeros; p.sigma2 = zeros; p.bearing = bearing; p.P3Dw = P3Dw; p.kp_index = kp;
  p.camera.model = ORBG_CAM_PINHOLE; p.camera.fx = 1.f; p.camera.fy = 1.f;
  std::vector<PnpJob> jobs(1);
  jobs[0] = PnpJob{&p, zeros, 1, 1, nullptr, R, t};
  PnpWork& w = batch_work();
  if ((rc = w.open(device, "misc"))) return rc;
  PnpOut o;
  if ((rc = launch(w, jobs, o))) return rc;
  memcpy(R_out, o.poses, 72); memcpy(t_out, o.poses + 9, 24);
  return ORBG_OK;
}
