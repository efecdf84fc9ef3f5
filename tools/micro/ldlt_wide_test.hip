// Stand-alone check + timing of csrc/ldlt_wide.hpp (k_wide_panel / k_wide_update / k_wide_back, launch_ldlt_wide: the many-workgroup
// LDL^T behind every reduced system of more than 50 free poses / 42 free keyframes).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o ldlt_wide_test ldlt_wide_test.hip && ./ldlt_wide_test
//   ./ldlt_wide_test bound [max n]   runs NO device code: a plain unblocked float64 LDL^T on the host against the same references, the
//                                    figures kF64 below holds the device to ten times of (8190 and 8192 take a minute or two each)
// References, none of them the code under test:
//   (a) "dense":  a dense random SPD matrix against an unblocked long-double LDL^T on the host, O(n^3): up to kDenseMax = 1542
//                 unknowns (the host side of the whole program then stays at a few seconds);
//   (b) "rank3":  S = D + U U^T, D a positive diagonal, U n x 3 dense random; the solution by Woodbury's identity in long double,
//                 O(n).  D and U are small dyadic rationals, so that the float64 matrix IS D + U U^T, not a rounding of it;
//   (c) the residual b - S x of every case, accumulated in long double, O(n^2).
// Every device buffer lies in an arena of the largest size with a guard band behind the part in use; the band is compared after every
// solve, x starts as a sentinel, the scratch as NaN, and b is compared with what was uploaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <map>
#include <random>
#include <vector>

namespace {
#include "../../multi_orbslam3_amd/csrc/ldlt_wide.hpp"

static_assert((size_t)kWideMaxUnknowns * sizeof(double) <= 65536, "k_wide_back keeps x in 64 KB of LDS");
static_assert(kWideMaxUnknowns == 8192, "the sizes below are written for a cap of 8192 unknowns");

#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); exit(2); } } while (0)

typedef long double ld;

constexpr int kDenseMax = 1542;

// the unblocked right-looking LDL^T + solve of ldlt_mfma_test's host_solve, in R = long double (reference) or double (bound)
template <class R>
bool host_ldlt(int n, const std::vector<double>& S, const std::vector<double>& b, std::vector<R>& y) {
  std::vector<R> a(S.begin(), S.end()), u(n);
  y.assign(b.begin(), b.end());
  for (int j = 0; j < n; j++) {
    const R d = a[(size_t)j * n + j];
    if (d == 0) return false;
    for (int c = j + 1; c < n; c++) u[c] = a[(size_t)c * n + j];          // the unscaled column
    for (int i = j + 1; i < n; i++) {
      R* row = &a[(size_t)i * n];
      const R l = u[i] / d;
      for (int c = j + 1; c <= i; c++) row[c] -= l * u[c];
      row[j] = l;
    }
  }
  for (int i = 0; i < n; i++) { const R* row = &a[(size_t)i * n]; R s = y[i]; for (int j = 0; j < i; j++) s -= row[j] * y[j]; y[i] = s; }
  for (int i = 0; i < n; i++) y[i] /= a[(size_t)i * n + i];
  for (int i = n - 1; i >= 0; i--) { const R xi = y[i]; const R* row = &a[(size_t)i * n]; for (int j = 0; j < i; j++) y[j] -= row[j] * xi; }
  return true;
}

enum Fam { DENSE = 0, RANK3 = 1, EGFIX = 2, INDEF = 3 };
const char* const kFamName[4] = {"dense", "rank3", "egfix", "indef"};

struct Sys { Fam fam; int n; std::vector<double> S, b; std::vector<ld> xr; };

// (a) a Wigner matrix (off-diagonal N(0, 1/n): spectrum within about [-2, 2]) plus a diagonal of 4 + |N(0, 1)|
Sys build_dense(int n) {
  Sys y; y.fam = DENSE; y.n = n; y.S.resize((size_t)n * n); y.b.resize(n);
  std::mt19937_64 rng(1000 + n);
  std::normal_distribution<double> N01(0.0, 1.0);
  const double sc = 1.0 / std::sqrt((double)n);
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < i; j++) y.S[(size_t)i * n + j] = y.S[(size_t)j * n + i] = sc * N01(rng);
    y.S[(size_t)i * n + i] = 4.0 + std::fabs(N01(rng));
  }
  for (auto& v : y.b) v = N01(rng);
  host_ldlt<ld>(n, y.S, y.b, y.xr);
  return y;
}

// (b) and the two structured variants of it.  U: multiples of 1/16 in [-2, 2]; D: multiples of 1/1024.
//   RANK3: D in [1, 2].
//   EGFIX: every seventh unknown (6, 13, ...) is a fixed-scale column of the essential graph: diagonal 1e-16 (lambda alone), row,
//          column and right-hand side 0.
//   INDEF: |D_i| = 1 + sum_j |u_i . u_j| (strictly dominant over row i of U U^T), the sign at random.
Sys build_rank(Fam fam, int n) {
  Sys y; y.fam = fam; y.n = n; y.S.resize((size_t)n * n); y.b.resize(n);
  std::mt19937_64 rng(2000 + 10 * (uint64_t)n + (int)fam);
  std::normal_distribution<double> N01(0.0, 1.0);
  std::vector<double> U((size_t)n * 3), D(n);
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) U[3 * i + k] = ((int)(rng() % 65) - 32) / 16.0;
    D[i] = (1024 + (int)(rng() % 1025)) / 1024.0;
    y.b[i] = N01(rng);
    if (fam == EGFIX && i % 7 == 6) { U[3 * i] = U[3 * i + 1] = U[3 * i + 2] = 0.0; D[i] = 1e-16; y.b[i] = 0.0; }
  }
  for (int i = 0; i < n; i++) {
    double* row = &y.S[(size_t)i * n];
    const double a = U[3 * i], b = U[3 * i + 1], c = U[3 * i + 2];
    for (int j = 0; j < n; j++) row[j] = a * U[3 * j] + b * U[3 * j + 1] + c * U[3 * j + 2];       // exact: multiples of 1/256, below 13
  }
  if (fam == INDEF)
    for (int i = 0; i < n; i++) {
      double s = 1.0;
      for (int j = 0; j < n; j++) s += std::fabs(y.S[(size_t)i * n + j]);                           // exact as well
      D[i] = (rng() & 1) ? s : -s;
    }
  for (int i = 0; i < n; i++) y.S[(size_t)i * n + i] += D[i];
  // Woodbury: x = D^-1 b - D^-1 U (I + U^T D^-1 U)^-1 U^T D^-1 b
  ld C[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
  for (int i = 0; i < n; i++)
    for (int p = 0; p < 3; p++) {
      for (int q = 0; q < 3; q++) C[p][q] += (ld)U[3 * i + p] * U[3 * i + q] / D[i];
      C[p][3] += (ld)U[3 * i + p] * y.b[i] / D[i];
    }
  for (int p = 0; p < 3; p++) {                                                                     // 3 x 3 elimination, partial pivoting
    int best = p;
    for (int q = p + 1; q < 3; q++) if (fabsl(C[q][p]) > fabsl(C[best][p])) best = q;
    for (int q = 0; q < 4; q++) std::swap(C[p][q], C[best][q]);
    for (int r = p + 1; r < 3; r++) { const ld f = C[r][p] / C[p][p]; for (int q = p; q < 4; q++) C[r][q] -= f * C[p][q]; }
  }
  ld w[3];
  for (int p = 2; p >= 0; p--) { ld s = C[p][3]; for (int q = p + 1; q < 3; q++) s -= C[p][q] * w[q]; w[p] = s / C[p][p]; }
  y.xr.resize(n);
  for (int i = 0; i < n; i++) y.xr[i] = ((ld)y.b[i] - (U[3 * i] * w[0] + U[3 * i + 1] * w[1] + U[3 * i + 2] * w[2])) / D[i];
  return y;
}

Sys build(Fam fam, int n) { return fam == DENSE ? build_dense(n) : build_rank(fam, n); }

// S = L D L^T in exact small integers: L unit lower with entries -1, 0, 1 in a band of 24 (it crosses the 16-column blocks), D powers
// of two of either sign, d_p = 0.  Every intermediate of an LDL^T of S, blocked or not, is an integer or an integer over a power
// of two, so the pivot at p is reached as exactly 0 in any order of summation.
void build_zero_pivot(int n, int p, std::vector<double>& S, std::vector<double>& b) {
  std::mt19937_64 rng(3000 + 10 * (uint64_t)n + p);
  const int bw = 24;
  std::vector<int> L((size_t)n * (bw + 1), 0), d(n);
  const int dv[6] = {1, 2, 4, -1, -2, -4};
  for (int i = 0; i < n; i++) {
    d[i] = i == p ? 0 : dv[rng() % 6];
    for (int k = 0; k < bw; k++) L[(size_t)i * (bw + 1) + k] = i - bw + k >= 0 ? (int)(rng() % 3) - 1 : 0;      // L[i][i - bw + k]
    L[(size_t)i * (bw + 1) + bw] = 1;
  }
  S.assign((size_t)n * n, 0.0); b.resize(n);
  for (int i = 0; i < n; i++)
    for (int j = std::max(0, i - bw); j <= i; j++) {
      int s = 0;
      for (int k = std::max(0, i - bw); k <= j; k++) s += L[(size_t)i * (bw + 1) + k - i + bw] * d[k] * L[(size_t)j * (bw + 1) + k - j + bw];
      S[(size_t)i * n + j] = S[(size_t)j * n + i] = s;
    }
  for (auto& v : b) v = (double)((int)(rng() % 17) - 8);
}

struct Fig { double err, res; };

// err = max|x - x_ref| / max|x_ref|, res = max|b - S x| / max|b| with the residual in long double
template <class X>
Fig figures(const Sys& y, const X* x) {
  const int n = y.n;
  ld mx = 0, e = 0, mb = 0, r = 0;
  for (int i = 0; i < n; i++) { mx = std::max(mx, fabsl(y.xr[i])); e = std::max(e, fabsl((ld)x[i] - y.xr[i])); mb = std::max(mb, fabsl((ld)y.b[i])); }
  for (int i = 0; i < n; i++) {
    const double* row = &y.S[(size_t)i * n];
    ld s = y.b[i];
    for (int j = 0; j < n; j++) s -= (ld)row[j] * (ld)x[j];
    r = std::max(r, fabsl(s));
  }
  return {(double)(e / mx), (double)(r / mb)};
}

// ---- the float64 host figures (./ldlt_wide_test bound), largest of a family over a band of sizes; {error, residual}.  The device is held
// to max(1e-10, 10 x figure): the blocked kernels sum in another order than the unblocked host code, and that is all that may differ.
constexpr int kBands = 7;
const int kBandMax[kBands] = {33, 320, 1030, 1542, 2049, 2994, 8192};
int band_of(int n) { int k = 0; while (n > kBandMax[k]) k++; return k; }
const Fig kF64[4][kBands] = {
    /* dense */ {{9.3e-16, 1.01e-15}, {3.46e-15, 2.94e-15}, {3.12e-15, 3.26e-15}, {7.6e-15, 7.76e-15}, {0, 0}, {0, 0}, {0, 0}},
    /* rank3 */ {{1.2e-15, 1.29e-15}, {3.79e-15, 1.05e-14}, {6.72e-15, 1.34e-14}, {6.82e-15, 1.92e-14}, {1.02e-14, 2.46e-14}, {1.12e-14, 3.9e-14}, {6.98e-14, 1.76e-13}},
    /* egfix */ {{0, 0}, {1.77e-15, 2.92e-15}, {4.88e-15, 1.82e-14}, {0, 0}, {0, 0}, {0, 0}, {0, 0}},
    /* indef */ {{0, 0}, {7.61e-16, 7.23e-16}, {2.35e-15, 3.46e-15}, {0, 0}, {0, 0}, {0, 0}, {0, 0}},
};
Fig bound_of(Fam fam, int n) {
  const Fig f = kF64[fam][band_of(n)];
  return {std::max(1e-10, 10.0 * f.err), std::max(1e-10, 10.0 * f.res)};
}

const int kSizes[] = {1, 15, 16, 17, 31, 32, 33, 304, 305, 306, 307, 308, 309, 310, 311, 312, 313, 314, 315, 316, 317, 318, 319, 320,
                      1023, 1024, 1025, 1542, 2049, 8190, 8192};
const int kStructSizes[] = {100, 1030};

int run_bound(int max_n) {
  Fig worst[4][kBands] = {};
  auto one = [&](Fam fam, int n) {
    if (n > max_n) return;
    const Sys y = build(fam, n);
    std::vector<double> x;
    const auto t0 = std::chrono::steady_clock::now();
    host_ldlt<double>(n, y.S, y.b, x);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const Fig f = figures(y, x.data());
    Fig& w = worst[fam][band_of(n)];
    w.err = std::max(w.err, f.err); w.res = std::max(w.res, f.res);
    printf("float64 host n=%4d %s: err %.3e res %.3e (%.1f s)\n", n, kFamName[fam], f.err, f.res, s);
    fflush(stdout);
  };
  for (int n : kSizes) { if (n <= kDenseMax) one(DENSE, n); one(RANK3, n); }
  for (int n : kStructSizes) { one(RANK3, n); one(EGFIX, n); one(INDEF, n); one(RANK3, 16 * ((n + 15) / 16)); }
  one(RANK3, 2994);
  for (int f = 0; f < 4; f++) {
    printf("/* %s */ {", kFamName[f]);
    for (int k = 0; k < kBands; k++) printf("{%.3g, %.3g}%s", worst[f][k].err, worst[f][k].res, k + 1 < kBands ? ", " : "},\n");
  }
  return 0;
}

// ---- the device side
constexpr int kCapN = kWideMaxUnknowns + 1;       // 8193 is offered (and refused)
constexpr int kGuard = 4096;                      // elements behind the part of a buffer in use
constexpr uint64_t kGuardBits = 0xA5A5A5A5A5A5A5A5ull, kSentinelBits = 0xDEADBEEFCAFEF00Dull;
constexpr int kGuardInt = (int)0xA5A5A5A5, kOkPreset = -1;

struct Arena { double *S, *S0, *b, *x, *w; int* ok; } A;
std::vector<uint64_t> g_guard(kGuard, kGuardBits);
std::vector<int> g_guard_int(kGuard, kGuardInt);

void arena_alloc() {
  CK(hipMalloc(&A.S, ((size_t)kCapN * kCapN + kGuard) * 8));
  CK(hipMalloc(&A.S0, (size_t)kCapN * kCapN * 8));
  CK(hipMalloc(&A.b, (size_t)(kCapN + kGuard) * 8));
  CK(hipMalloc(&A.x, (size_t)(kCapN + kGuard) * 8));
  CK(hipMalloc(&A.w, (size_t)(2 * kCapN + kGuard) * 8));
  CK(hipMalloc(&A.ok, (size_t)(1 + kGuard) * 4));
  const int pre = kOkPreset;
  CK(hipMemcpy(A.ok, &pre, 4, hipMemcpyHostToDevice));
}

struct Run { hipError_t err; int ok; std::vector<double> x; bool guards, b_same, x_untouched; };

bool guard_intact(const void* dev, size_t bytes, const void* pattern) {
  std::vector<unsigned char> h(bytes);
  CK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
  return memcmp(h.data(), pattern, bytes) == 0;
}

// one launch_ldlt_wide on fresh copies.  S may be empty (n = 8193: nothing is uploaded, nothing may be launched); preset_ok = false
// leaves the flag word as the solve before left it
Run solve(int n, const std::vector<double>& S, const std::vector<double>& b, bool preset_ok = true) {
  const size_t nn = (size_t)n * n;
  std::vector<uint64_t> sent(n, kSentinelBits);
  std::vector<double> nans(2 * (size_t)n, std::nan(""));
  if (!S.empty()) CK(hipMemcpy(A.S, S.data(), nn * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.S + nn, g_guard.data(), kGuard * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.b, b.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.b + n, g_guard.data(), kGuard * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.x, sent.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.x + n, g_guard.data(), kGuard * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.w, nans.data(), 2 * (size_t)n * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.w + 2 * (size_t)n, g_guard.data(), kGuard * 8, hipMemcpyHostToDevice));
  const int pre = kOkPreset;
  if (preset_ok) CK(hipMemcpy(A.ok, &pre, 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.ok + 1, g_guard_int.data(), kGuard * 4, hipMemcpyHostToDevice));
  Run r;
  r.err = launch_ldlt_wide(n, A.S, A.b, A.x, A.ok, A.w, 0);
  CK(hipDeviceSynchronize());
  r.x.resize(n);
  std::vector<double> b2(n);
  CK(hipMemcpy(r.x.data(), A.x, (size_t)n * 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(&r.ok, A.ok, 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(b2.data(), A.b, (size_t)n * 8, hipMemcpyDeviceToHost));
  r.b_same = memcmp(b2.data(), b.data(), (size_t)n * 8) == 0;
  r.x_untouched = memcmp(r.x.data(), sent.data(), (size_t)n * 8) == 0;
  r.guards = guard_intact(A.S + nn, kGuard * 8, g_guard.data()) & guard_intact(A.b + n, kGuard * 8, g_guard.data()) &
             guard_intact(A.x + n, kGuard * 8, g_guard.data()) & guard_intact(A.w + 2 * (size_t)n, kGuard * 8, g_guard.data()) &
             guard_intact(A.ok + 1, kGuard * 4, g_guard_int.data());
  return r;
}

Fig g_dev[4][kBands] = {};

// a good solve against the reference of its system: flag, both figures within ten times the float64 host's, guards, b
bool good_solve(const Sys& y, const Run& r, Fig* out = nullptr) {
  const Fig f = figures(y, r.x.data()), bd = bound_of(y.fam, y.n);
  Fig& w = g_dev[y.fam][band_of(y.n)];
  if (f.err == f.err) w.err = std::max(w.err, f.err);
  if (f.res == f.res) w.res = std::max(w.res, f.res);
  if (out) *out = f;
  return r.err == hipSuccess && r.ok == 1 && f.err <= bd.err && f.res <= bd.res && r.guards && r.b_same;
}

// microseconds per solve: three solves after one warm-up, each from a fresh device copy of S, HIP events round the solve alone
double time_solves(const Sys& y) {
  const int n = y.n;
  const size_t nn = (size_t)n * n;
  CK(hipMemcpy(A.S0, y.S.data(), nn * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(A.b, y.b.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  double us = 0;
  for (int it = 0; it < 4; it++) {
    CK(hipMemcpyAsync(A.S, A.S0, nn * 8, hipMemcpyDeviceToDevice, 0));
    CK(hipEventRecord(e0, 0));
    CK(launch_ldlt_wide(n, A.S, A.b, A.x, A.ok, A.w, 0));
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (it) us += 1000.0 * ms;
  }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return us / 3;
}

int run_device() {
  int fails = 0;
  arena_alloc();
  // ---- sizes, each the smallest that reaches its path: one block (padded or not), T = 2 and 3, all sixteen residues of the last block
  // just past the matrix-core limit, the second lap of k_wide_back's strided loops, the largest system of the library's own tests,
  // 2049, both caps of the callers (8190) and the solver's own (8192)
  std::map<int, std::future<Sys>> ahead;            // the long-double factorisations of the four largest dense systems, side by side
  for (int n : kSizes) if (n > 1000 && n <= kDenseMax) ahead[n] = std::async(std::launch::async, build_dense, n);
  for (int n : kSizes)
    for (Fam fam : {DENSE, RANK3}) {
      if (fam == DENSE && n > kDenseMax) continue;
      const Sys y = fam == DENSE && ahead.count(n) ? ahead[n].get() : build(fam, n);
      const Run r = solve(n, y.S, y.b);
      Fig f;
      const bool good = good_solve(y, r, &f);
      const Fig bd = bound_of(fam, n);
      printf("n=%4d %s T=%3d ok=%d err %.3e (<= %.1e) res %.3e (<= %.1e) guards %d b %d %s\n", n, kFamName[fam], (n + 15) / 16, r.ok, f.err, bd.err, f.res,
             bd.res, (int)r.guards, (int)r.b_same, good ? "ok" : "FAIL");
      fails += !good;
      if (fam == RANK3 && (n == 320 || n == 1025 || n == 8190)) {        // equal bits: a second solve from fresh copies
        const Run r2 = solve(n, y.S, y.b);
        const bool same = r2.ok == r.ok && memcmp(r2.x.data(), r.x.data(), (size_t)n * 8) == 0 && r2.guards;
        printf("bits n=%d: two solves %s %s\n", n, same ? "equal" : "DIFFER", same ? "ok" : "FAIL");
        fails += !same;
      }
      if (fam == RANK3 && (n == 320 || n == 1542 || n == 8190)) printf("time n=%d: %.1f us per solve\n", n, time_solves(y));
      fflush(stdout);
    }
  {   // one above the cap: refused before anything is launched
    const int n = kWideMaxUnknowns + 1;
    const std::vector<double> b(n, 1.0);
    const Run r = solve(n, std::vector<double>(), b);
    const bool good = r.err == hipErrorInvalidValue && r.x_untouched && r.ok == kOkPreset && r.guards && r.b_same;
    printf("refusal n=%d: %s, x untouched %d ok word %d guards %d %s\n", n, hipGetErrorName(r.err), (int)r.x_untouched, r.ok, (int)r.guards, good ? "ok" : "FAIL");
    fails += !good;
  }
  {   // the size of the 500-keyframe full BA (499 free poses): checked like the others, here for its time
    const Sys y = build(RANK3, 2994);
    const Run r = solve(y.n, y.S, y.b);
    Fig f;
    const bool good = good_solve(y, r, &f);
    printf("extra n=%d rank3 ok=%d err %.3e res %.3e %s\n", y.n, r.ok, f.err, f.res, good ? "ok" : "FAIL");
    fails += !good;
    printf("time n=%d: %.1f us per solve\n", y.n, time_solves(y));
  }
  // ---- structure, at one size below and one above k_wide_back's first lap, both with a padded last block (100 = 6 x 16 + 4, 1030 = 64 x 16 + 6)
  for (int n : kStructSizes) {
    const Sys yg = build(RANK3, n);
    const Run rg = solve(n, yg.S, yg.b);
    {
      const bool good = good_solve(yg, rg);
      printf("struct n=%d rank3 itself: ok=%d %s\n", n, rg.ok, good ? "ok" : "FAIL");
      fails += !good;
    }
    {   // the essential graph's fixed-scale columns
      const Sys y = build(EGFIX, n);
      const Run r = solve(n, y.S, y.b);
      Fig f;
      bool good = good_solve(y, r, &f);
      int nonzero = 0;
      for (int i = 6; i < n; i += 7) nonzero += !(r.x[i] == 0.0);
      good = good && nonzero == 0;
      printf("egfix n=%d: ok=%d err %.3e res %.3e, %d fixed unknowns not exactly 0 %s\n", n, r.ok, f.err, f.res, nonzero, good ? "ok" : "FAIL");
      fails += !good;
    }
    {   // indefinite and well conditioned: only a zero or non-finite pivot fails
      const Sys y = build(INDEF, n);
      const Run r = solve(n, y.S, y.b);
      Fig f;
      const bool good = good_solve(y, r, &f);
      printf("indef n=%d: ok=%d err %.3e res %.3e %s\n", n, r.ok, f.err, f.res, good ? "ok" : "FAIL");
      fails += !good;
    }
    {   // the reading contract: the strictly lower triangle of every diagonal block and every block above the diagonal are never input
      std::vector<double> P = yg.S;
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
          const int bi = i >> 4, bj = j >> 4;
          if (bj > bi || (bi == bj && j < i)) P[(size_t)i * n + j] = std::nan("");
        }
      const Run r = solve(n, P, yg.b);
      const bool same = r.err == hipSuccess && r.ok == rg.ok && memcmp(r.x.data(), rg.x.data(), (size_t)n * 8) == 0 && r.guards && r.b_same;
      printf("contract n=%d: NaN where the kernels may not read: ok=%d, x %s %s\n", n, r.ok, same ? "equal bits" : "DIFFERS", same ? "ok" : "FAIL");
      fails += !same;
    }
    // failing pivots: flag cleared, x left alone; then a good system on the same flag word
    const int mid = 16 * ((n + 15) / 32) + 5;
    const int at[5] = {0, 7, 16, mid, n - 1};
    auto failing = [&](const Sys& good, const Run& good_run, const std::vector<double>& S, const std::vector<double>& b, const char* what) {
      const int m = good.n;
      const Run r = solve(m, S, b);
      const Run r2 = solve(m, good.S, good.b, /*preset_ok*/ false);
      const bool failed = r.err == hipSuccess && r.ok == 0 && r.x_untouched && r.guards && r.b_same;
      const bool after = good_solve(good, r2) && memcmp(r2.x.data(), good_run.x.data(), (size_t)m * 8) == 0;
      printf("pivot n=%d %s: ok=%d x untouched %d guards %d; the next solve on the same flag: ok=%d %s\n", m, what, r.ok, (int)r.x_untouched, (int)r.guards, r2.ok,
             failed && after ? "ok" : "FAIL");
      fails += !(failed && after);
    };
    for (int k = 0; k < 7; k++) {
      std::vector<double> S, b;
      char what[64];
      if (k < 5) { build_zero_pivot(n, at[k], S, b); snprintf(what, sizeof what, "pivot %d exactly 0", at[k]); }
      else { S = yg.S; b = yg.b; S[(size_t)mid * n + mid] = k == 5 ? std::nan("") : (double)INFINITY; snprintf(what, sizeof what, "S[%d][%d] = %s", mid, mid, k == 5 ? "NaN" : "+Inf"); }
      failing(yg, rg, S, b, what);
    }
    {   // the last pivot of a FULL last block: the one zero pivot that no non-finite pivot follows (everywhere else, the padding of
        // the last block included, 0 / 0 reaches a later pivot, and the test for NaN would flag the factorisation by itself)
      const int nf = 16 * ((n + 15) / 16);
      const Sys yf = build(RANK3, nf);
      const Run rf = solve(nf, yf.S, yf.b);
      const bool good = good_solve(yf, rf);
      printf("struct n=%d rank3 itself: ok=%d %s\n", nf, rf.ok, good ? "ok" : "FAIL");
      fails += !good;
      std::vector<double> S, b;
      char what[64];
      build_zero_pivot(nf, nf - 1, S, b);
      snprintf(what, sizeof what, "pivot %d exactly 0, last of a full block", nf - 1);
      failing(yf, rf, S, b, what);
    }
    fflush(stdout);
  }
  for (int f = 0; f < 4; f++) {
    printf("device %s by band {err, res}:", kFamName[f]);
    for (int k = 0; k < kBands; k++) printf(" <=%d {%.3g, %.3g}", kBandMax[k], g_dev[f][k].err, g_dev[f][k].res);
    printf("\n");
  }
  printf(fails ? "FAILED (%d)\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "bound")) return run_bound(argc > 2 ? atoi(argv[2]) : 1 << 30);
  return run_device();
}
