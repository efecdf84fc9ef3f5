// The shared device primitives of csrc/ evaluated one by one: wave.hpp, lm_block.hpp, lm_record.hpp, lm_step.hpp, se3.hpp,
// sim3_math.hpp, pose_inertial_edges.hpp, null_vector4.hpp.  This program holds no test data and no copy of any function under test: it reads a file of
// cases, calls the headers' functions and writes what they returned.  tests/device_math_model.py makes the cases and the expected values.
//
//   device_math_test [host] CASES OUT
//
// `host`: no HIP call is made; only the __host__ __device__ functions are evaluated (on the CPU), every other case gets zero outputs.
// Without it every function runs on the device: one kernel per family, wavefront primitives in 64-thread workgroups (one case per
// workgroup), block primitives in 256-thread workgroups, the lane solve on one wavefront per case with lanes N..63 holding NaN, the
// scalar functions one case per thread.  A HIP call that fails prints its error and the program exits 3 without another launch.
//
// CASES (little endian):  int32 magic 0x444d5431, int32 n_cases, then per case
//     int32 fid, int32 n_int, int32 n_dbl, int32 pad(0), n_int x int32 (padded with one int32 when n_int is odd), n_dbl x float64
// OUT:                    int32 magic 0x444d5432, int32 n_cases, then per case
//     int32 fid, int32 n_out, n_out x float64          (n_out = 0: not evaluated in this mode)
// Integer results are written as the float64 of their value (exact).  The inputs and outputs of every fid are the rows of kFns below;
// a case whose counts differ from its row is refused (exit 2) before anything runs.
//
//   fid  function                     in                                                       out
//     1  wave int primitives          64 int32 (lane values)                                   6 x 64: incl_scan_add(int), wave_sum(int), wave_max,
//                                                                                              wave_min(unsigned), incl_scan_add(unsigned), wave_sum(unsigned), per lane
//     2  wave_sum_f64                 64 f64                                                   64 (per lane)
//     3  block_sum                    2 x 256 f64 (first call slot 0, second call slot 1)      2 x 256 (per thread)
//     4  block_sum_256                256 f64                                                  1 (thread 0)
//     5  lm_block_reduce<28>          256 x 28 f64 (thread-major)                              28
//  10-15 lane_ldlt_solve <6> <7> <9,false> <9,true> <15,true> <30,true>
//                                     N x N H row-major, N b, lambda, sentinel                 ok(lane 0), ok(lane 63), x[N] of lane 0, x[N] of lane 63
//    20  quat_from_R  9 -> 4      21  quat_to_R  4 -> 9      22  quat_rotate  q4 v3 -> 3      23  quat_normalize  4 -> 4
//    24  se3_mul  a(q4 t3) b(q4 t3) -> q4 t3                 25  s3_mul  a(q4 t3 s) b(q4 t3 s) -> q4 t3 s
//    26  s3_inverse  q4 t3 s -> q4 t3 s                      27  s3_map  q4 t3 s X3 -> 3
//    28  s3_exp  7 -> q4 t3 s                                29  s3_log  q4 t3 s -> 7
//    30  pose_oplus  T(q4 t3) u6 -> q4 t3      31  pose_oplus_fast  same      32  pose_oplus_series  same
//    33  fast_rsqrt  1 -> 1
//    34  cam_project  model fx fy cx cy k1 k2 k3 k4 v3 -> 2  35  cam_project_jac  same -> 6
//    40  pi_exp_so3  3 -> 9       41  pi_log_so3  9 -> 3     42  pi_right_jacobian  3 -> 9    43  pi_inv_right_jacobian  3 -> 9
//    44  pi_normalize_rotation  9 -> 9          45  pi_gdir_oplus  Rwg9 u0 u1 -> 9
//    46  pi_oplus  R9 t3 v3 bg3 ba3 dx15 -> R9 t3 v3 bg3 ba3
//    50  null_vector4  16 (S row-major) -> v4, S diagonal 4 (after the sweeps)
//    60  lm_trial_verdict  lambda ni currentChi solver_ok chi2_trial scale -> rho accepted lambda ni currentChi
//    61  lm_accepted_lambda  lambda rho -> 1                62  lm_iteration_continues  currentChi nBad trials_exhausted rho iniChi -> continues nBad
//    63  lm_lambda_init  user max_diagonal -> 1             64  lm_huber  e delta dsqr -> rho0 rho1
//        (60, 64: a NaN result is written as -777.25, so that the host's and the device's NaN need not share a payload)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (found through -I multi_orbslam3_amd/csrc)
#include "se3.hpp"
#include "sim3_math.hpp"
#include "lm_block.hpp"
#include "lm_record.hpp"
#include "lm_step.hpp"
#include "null_vector4.hpp"
namespace {
#include "pose_inertial_edges.hpp"
}

#define CHECK(call)                                                                                         \
  do {                                                                                                      \
    const hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__, #call); exit(3); } \
  } while (0)

namespace {

using namespace orbg_se3;
using namespace orbg_s3;

struct Fn { int fid, n_int, n_dbl, n_out, hd; };
constexpr Fn kFns[] = {
    {1, 64, 0, 384, 0},   {2, 0, 64, 64, 0},    {3, 0, 512, 512, 0},  {4, 0, 256, 1, 0},    {5, 0, 256 * 28, 28, 0},
    {10, 0, 44, 14, 0},   {11, 0, 58, 16, 0},   {12, 0, 92, 20, 0},   {13, 0, 92, 20, 0},   {14, 0, 242, 32, 0},  {15, 0, 932, 62, 0},
    {20, 0, 9, 4, 1},     {21, 0, 4, 9, 1},     {22, 0, 7, 3, 1},     {23, 0, 4, 4, 1},     {24, 0, 14, 7, 1},    {25, 0, 16, 8, 1},
    {26, 0, 8, 8, 1},     {27, 0, 11, 3, 1},    {28, 0, 7, 8, 1},     {29, 0, 8, 7, 1},     {30, 0, 13, 7, 0},    {31, 0, 13, 7, 0},
    {32, 0, 13, 7, 0},    {33, 0, 1, 1, 0},     {34, 0, 12, 2, 0},    {35, 0, 12, 6, 0},    {40, 0, 3, 9, 1},     {41, 0, 9, 3, 1},
    {42, 0, 3, 9, 1},     {43, 0, 3, 9, 1},     {44, 0, 9, 9, 1},     {45, 0, 11, 9, 1},    {46, 0, 36, 21, 1},   {50, 0, 16, 8, 0},
    {60, 0, 6, 5, 1},     {61, 0, 2, 1, 1},     {62, 0, 5, 2, 1},     {63, 0, 2, 1, 1},     {64, 0, 3, 2, 1},
};
const Fn* find_fn(int fid) {
  for (const Fn& f : kFns) if (f.fid == fid) return &f;
  return nullptr;
}

// ---- the __host__ __device__ functions: one evaluator for the CPU mode and for the scalar kernel
__host__ __device__ inline void load_pose(const double* p, PoseQ* T) { for (int i = 0; i < 4; i++) T->q[i] = p[i]; for (int i = 0; i < 3; i++) T->t[i] = p[4 + i]; }
__host__ __device__ inline void store_pose(const PoseQ& T, double* p) { for (int i = 0; i < 4; i++) p[i] = T.q[i]; for (int i = 0; i < 3; i++) p[4 + i] = T.t[i]; }
__host__ __device__ inline void load_s3(const double* p, S3* T) { for (int i = 0; i < 4; i++) T->q[i] = p[i]; for (int i = 0; i < 3; i++) T->t[i] = p[4 + i]; T->s = p[7]; }
__host__ __device__ inline void store_s3(const S3& T, double* p) { for (int i = 0; i < 4; i++) p[i] = T.q[i]; for (int i = 0; i < 3; i++) p[4 + i] = T.t[i]; p[7] = T.s; }

__host__ __device__ inline double nan_as_sentinel(double v) { return v == v ? v : -777.25; }

__host__ __device__ inline void eval_hd(int fid, const double* in, double* out) {
  switch (fid) {
    case 20: quat_from_R(in, out); break;
    case 21: quat_to_R(in, out); break;
    case 22: quat_rotate(in, in + 4, out); break;
    case 23: { for (int i = 0; i < 4; i++) out[i] = in[i]; quat_normalize(out); break; }
    case 24: { PoseQ a, b, o; load_pose(in, &a); load_pose(in + 7, &b); se3_mul(a, b, &o); store_pose(o, out); break; }
    case 25: { S3 a, b, o; load_s3(in, &a); load_s3(in + 8, &b); s3_mul(a, b, &o); store_s3(o, out); break; }
    case 26: { S3 a, o; load_s3(in, &a); s3_inverse(a, &o); store_s3(o, out); break; }
    case 27: { S3 a; load_s3(in, &a); s3_map(a, in + 8, out); break; }
    case 28: { S3 o; s3_exp(in, &o); store_s3(o, out); break; }
    case 29: { S3 a; load_s3(in, &a); s3_log(a, out); break; }
    case 40: pi_exp_so3(in, out); break;
    case 41: pi_log_so3(in, out); break;
    case 42: pi_right_jacobian(in, out); break;
    case 43: pi_inv_right_jacobian(in, out); break;
    case 44: { for (int i = 0; i < 9; i++) out[i] = in[i]; pi_normalize_rotation(out); break; }
    case 45: { for (int i = 0; i < 9; i++) out[i] = in[i]; pi_gdir_oplus(out, in[9], in[10]); break; }
    case 46: {
      PiState s;
      for (int i = 0; i < 9; i++) s.R[i] = in[i];
      for (int i = 0; i < 3; i++) { s.t[i] = in[9 + i]; s.v[i] = in[12 + i]; s.bg[i] = in[15 + i]; s.ba[i] = in[18 + i]; }
      pi_oplus(&s, in + 21);
      for (int i = 0; i < 9; i++) out[i] = s.R[i];
      for (int i = 0; i < 3; i++) { out[9 + i] = s.t[i]; out[12 + i] = s.v[i]; out[15 + i] = s.bg[i]; out[18 + i] = s.ba[i]; }
      break;
    }
    case 60: {
      orbg_lm::LmScalars m;
      m.lambda = in[0]; m.ni = in[1]; m.currentChi = in[2];
      bool accepted = false;
      out[0] = nan_as_sentinel(orbg_lm::lm_trial_verdict(m, in[3] != 0, in[4], in[5], &accepted));
      out[1] = accepted ? 1.0 : 0.0; out[2] = m.lambda; out[3] = m.ni; out[4] = m.currentChi;
      break;
    }
    case 61: out[0] = orbg_lm::lm_accepted_lambda(in[0], in[1]); break;
    case 62: {
      orbg_lm::LmScalars m;
      m.currentChi = in[0]; m.nBad = (int)in[1];
      out[0] = orbg_lm::lm_iteration_continues(m, in[2] != 0, in[3], in[4]) ? 1.0 : 0.0;
      out[1] = (double)m.nBad;
      break;
    }
    case 63: out[0] = orbg_lm::lm_lambda_init(in[0], in[1]); break;
    case 64: {
      double r0, r1;
      orbg_lm::lm_huber(in[0], in[1], in[2], &r0, &r1);
      out[0] = nan_as_sentinel(r0); out[1] = nan_as_sentinel(r1);
      break;
    }
    default: break;
  }
}

// ---- the device-only scalar functions
__device__ inline void eval_dev(int fid, const double* in, double* out) {
  switch (fid) {
    case 30: case 31: case 32: {
      PoseQ T, o;
      load_pose(in, &T);
      if (fid == 30) pose_oplus(T, in + 7, &o); else if (fid == 31) pose_oplus_fast(T, in + 7, &o); else pose_oplus_series(T, in + 7, &o);
      store_pose(o, out);
      break;
    }
    case 33: out[0] = fast_rsqrt(in[0]); break;
    case 34: case 35: {
      const CamModelD m{(int)in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8]};
      if (fid == 34) cam_project(m, in + 9, out); else cam_project_jac(m, in + 9, out);
      break;
    }
    case 50: {
      double S[4][4], v[4];
      for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) S[i][j] = in[4 * i + j];
      orbg::null_vector4(S, v);
      for (int i = 0; i < 4; i++) { out[i] = v[i]; out[4 + i] = S[i][i]; }
      break;
    }
    default: break;
  }
}

// one case per thread; the cases of one launch share fid, n_in and n_out
__global__ void k_scalar_hd(int fid, int n, int n_in, int n_out, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) eval_hd(fid, in + (size_t)i * n_in, out + (size_t)i * n_out);
}
__global__ void k_scalar_dev(int fid, int n, int n_in, int n_out, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) eval_dev(fid, in + (size_t)i * n_in, out + (size_t)i * n_out);
}

// ---- wavefront primitives: one 64-thread workgroup per case, every lane active
__global__ __launch_bounds__(64) void k_wave_int(const int* __restrict__ in, double* __restrict__ out) {
  const int l = threadIdx.x;
  const int v = in[blockIdx.x * 64 + l];
  double* o = out + (size_t)blockIdx.x * 384;
  o[l] = (double)orbg::wave_incl_scan_add(v);
  o[64 + l] = (double)orbg::wave_sum(v);
  o[128 + l] = (double)orbg::wave_max(v);
  o[192 + l] = (double)orbg::wave_min((unsigned)v);
  o[256 + l] = (double)orbg::wave_incl_scan_add((unsigned)v);
  o[320 + l] = (double)orbg::wave_sum((unsigned)v);
}
__global__ __launch_bounds__(64) void k_wave_f64(const double* __restrict__ in, double* __restrict__ out) {
  const int l = threadIdx.x;
  out[blockIdx.x * 64 + l] = orbg::wave_sum_f64(in[blockIdx.x * 64 + l]);
}

// ---- block primitives: one 256-thread workgroup per case
__global__ __launch_bounds__(256) void k_block_sum(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double s_wsum[2][4];
  const int t = threadIdx.x;
  const double* p = in + (size_t)blockIdx.x * 512;
  int slot = 0;
  const double a = orbg::block_sum(p[t], s_wsum, slot); slot ^= 1;        // two consecutive calls, as the solve kernels make them
  const double b = orbg::block_sum(p[256 + t], s_wsum, slot); slot ^= 1;
  out[(size_t)blockIdx.x * 512 + t] = a;
  out[(size_t)blockIdx.x * 512 + 256 + t] = b;
}
__global__ __launch_bounds__(256) void k_block_sum_256(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double red[4];
  const double s = orbg_lm::block_sum_256(in[(size_t)blockIdx.x * 256 + threadIdx.x], red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}
template <int NV>
__global__ __launch_bounds__(256) void k_lm_reduce(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double s_acc[NV * orbg::kLmRow], s_part[NV * 8], s_out[NV];
  double vals[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) vals[v] = in[((size_t)blockIdx.x * 256 + threadIdx.x) * NV + v];
  orbg::lm_block_reduce<NV>(vals, s_acc, s_part, s_out);
  if (threadIdx.x >= 256 - NV) out[(size_t)blockIdx.x * NV + (threadIdx.x - (256 - NV))] = s_out[threadIdx.x - (256 - NV)];   // read by the LAST threads: valid for every thread
}

// ---- the lane solve: one wavefront per case, lane li holds row li, lanes N..63 hold NaN
template <int N, bool REL>
__global__ __launch_bounds__(64) void k_ldlt(const double* __restrict__ in, double* __restrict__ out) {
  constexpr int NIN = N * N + N + 2, NOUT = 2 * N + 2;
  const double* p = in + (size_t)blockIdx.x * NIN;
  const int li = threadIdx.x;
  const double lambda = p[N * N + N], sentinel = p[N * N + N + 1];
  double Hrow[N], x[N];
#pragma unroll
  for (int j = 0; j < N; j++) { Hrow[j] = li < N ? p[li * N + j] : NAN; x[j] = sentinel; }
  const double b = li < N ? p[N * N + li] : NAN;
  const bool ok = orbg::lane_ldlt_solve<N, REL>(Hrow, b, li, lambda, x);
  double* o = out + (size_t)blockIdx.x * NOUT;
  if (li == 0) { o[0] = ok ? 1.0 : 0.0; for (int j = 0; j < N; j++) o[2 + j] = x[j]; }
  if (li == 63) { o[1] = ok ? 1.0 : 0.0; for (int j = 0; j < N; j++) o[2 + N + j] = x[j]; }
}

struct Case { int fid; std::vector<int> iv; std::vector<double> dv; std::vector<double> out; };

template <class T>
T* to_device(const std::vector<T>& h) {
  T* d = nullptr;
  CHECK(hipMalloc(&d, h.size() * sizeof(T) + 8));
  CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

void run_group_on_device(const Fn& f, std::vector<Case*>& cs) {
  const int n = (int)cs.size();
  std::vector<double> hin;
  std::vector<int> hint;
  for (Case* c : cs) { hin.insert(hin.end(), c->dv.begin(), c->dv.end()); hint.insert(hint.end(), c->iv.begin(), c->iv.end()); }
  std::vector<double> hout((size_t)n * f.n_out, 0.0);
  double* din = to_device(hin);
  int* dint = to_device(hint);
  double* dout = to_device(hout);
  switch (f.fid) {
    case 1: k_wave_int<<<n, 64>>>(dint, dout); break;
    case 2: k_wave_f64<<<n, 64>>>(din, dout); break;
    case 3: k_block_sum<<<n, 256>>>(din, dout); break;
    case 4: k_block_sum_256<<<n, 256>>>(din, dout); break;
    case 5: k_lm_reduce<28><<<n, 256>>>(din, dout); break;
    case 10: k_ldlt<6, false><<<n, 64>>>(din, dout); break;
    case 11: k_ldlt<7, false><<<n, 64>>>(din, dout); break;
    case 12: k_ldlt<9, false><<<n, 64>>>(din, dout); break;
    case 13: k_ldlt<9, true><<<n, 64>>>(din, dout); break;
    case 14: k_ldlt<15, true><<<n, 64>>>(din, dout); break;
    case 15: k_ldlt<30, true><<<n, 64>>>(din, dout); break;
    default:
      if (f.hd) k_scalar_hd<<<(n + 63) / 64, 64>>>(f.fid, n, f.n_dbl, f.n_out, din, dout);
      else k_scalar_dev<<<(n + 63) / 64, 64>>>(f.fid, n, f.n_dbl, f.n_out, din, dout);
  }
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(hout.data(), dout, hout.size() * sizeof(double), hipMemcpyDeviceToHost));
  CHECK(hipFree(din));
  CHECK(hipFree(dint));
  CHECK(hipFree(dout));
  for (int i = 0; i < n; i++) cs[i]->out.assign(hout.begin() + (size_t)i * f.n_out, hout.begin() + (size_t)(i + 1) * f.n_out);
}

}  // namespace

int main(int argc, char** argv) {
  const bool host = argc > 1 && !strcmp(argv[1], "host");
  if (argc != (host ? 4 : 3)) { fprintf(stderr, "usage: %s [host] CASES OUT\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[host ? 2 : 1], "rb");
  if (!fi) { fprintf(stderr, "cannot read %s\n", argv[host ? 2 : 1]); return 2; }
  int head[2];
  if (fread(head, 4, 2, fi) != 2 || head[0] != 0x444d5431 || head[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<Case> cases(head[1]);
  for (Case& c : cases) {
    int h[4];
    if (fread(h, 4, 4, fi) != 4) { fprintf(stderr, "truncated case header\n"); return 2; }
    const Fn* f = find_fn(h[0]);
    if (!f || h[1] != f->n_int || h[2] != f->n_dbl) { fprintf(stderr, "case of fid %d with %d ints, %d doubles: not in the table\n", h[0], h[1], h[2]); return 2; }
    c.fid = h[0];
    c.iv.resize(h[1] + (h[1] & 1));
    c.dv.resize(h[2]);
    if (fread(c.iv.data(), 4, c.iv.size(), fi) != c.iv.size() || fread(c.dv.data(), 8, c.dv.size(), fi) != c.dv.size()) { fprintf(stderr, "truncated case\n"); return 2; }
    c.iv.resize(h[1]);
  }
  fclose(fi);

  for (const Fn& f : kFns) {
    std::vector<Case*> cs;
    for (Case& c : cases) if (c.fid == f.fid) cs.push_back(&c);
    if (cs.empty()) continue;
    if (host) {
      if (!f.hd) continue;
      for (Case* c : cs) { c->out.assign(f.n_out, 0.0); eval_hd(f.fid, c->dv.data(), c->out.data()); }
    } else {
      run_group_on_device(f, cs);
    }
    printf("fid %2d: %zu cases\n", f.fid, cs.size());
  }

  FILE* fo = fopen(argv[host ? 3 : 2], "wb");
  if (!fo) { fprintf(stderr, "cannot write %s\n", argv[host ? 3 : 2]); return 2; }
  const int ohead[2] = {0x444d5432, (int)cases.size()};
  fwrite(ohead, 4, 2, fo);
  for (const Case& c : cases) {
    const int h[2] = {c.fid, (int)c.out.size()};
    fwrite(h, 4, 2, fo);
    fwrite(c.out.data(), 8, c.out.size(), fo);
  }
  if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
  printf("%s: %zu cases done\n", host ? "host" : "device", cases.size());
  return 0;
}
