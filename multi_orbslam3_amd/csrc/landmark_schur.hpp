// The landmark-Schur pipeline between an edge kernel and the LDL^T of the full / welding BA (full_ba.hip) and the inertial local BA
// (inertial_ba.hip), written once: Hll, bl of a point from its run of edges, (Hll + lambda I)^-1, the reduction that ends a free pose's
// Hpp | bp, a pose pair's items into the 6 x 6 block -sum Hpl Dinv Hpl^T (| Hpl Dinv bl), an entry of the reduced system with its mirror
// image, the back-substitution of a point, and the host's check of the edge order all of it relies on.  No include guard and no
// namespace of its own: each translation unit includes it ONCE inside its anonymous namespace (the kernels are __global__ functions of
// that unit), after wave.hpp and ldlt_mfma.hpp.
//
// An edge's block is STRIDE doubles whose first 27 are Hpl (6 x 3, row-major, 18) | Hll upper (6) | bl (3) in both solves; what a solve
// appends (the inertial BA: Hpp | bp of the edge) only changes the stride.  A point's edges are consecutive in the edge list, and every
// sum below runs in a fixed order: the bits of a result do not depend on the launch.

constexpr int kSchurThreads = 256;      // workgroup size of every kernel that uses this header = the lap of its strided loops
constexpr int kSchurHll = 18;           // offset of Hll | bl in an edge's block
constexpr int kSchurHead = 27;          // doubles of an edge's block that are read here

struct SchurItem { int ea, eb; };       // edges (pose i / pose j) of one landmark both poses observe

// Hll, bl of every point: its edges in order
template <int STRIDE>
__global__ __launch_bounds__(256) void k_schur_points(int NX, const int* __restrict__ pt_start, const int* __restrict__ pt_end,
                                                      const double* __restrict__ EB, double* __restrict__ Hll, double* __restrict__ bl) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= NX) return;
  double acc[9];
#pragma unroll
  for (int i = 0; i < 9; i++) acc[i] = 0;
  for (int k = pt_start[l]; k < pt_end[l]; k++) {
    const double* eb = EB + (size_t)k * STRIDE + kSchurHll;
#pragma unroll
    for (int i = 0; i < 9; i++) acc[i] += eb[i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) Hll[6 * (size_t)l + i] = acc[i];
#pragma unroll
  for (int i = 0; i < 3; i++) bl[3 * (size_t)l + i] = acc[6 + i];
}

// Eigen-style cofactor inverse of (Hll + lambda I), upper six entries, and its product with bl
__global__ __launch_bounds__(256) void k_schur_dinv(int NX, const double* __restrict__ Hll, const double* __restrict__ bl, double lambda,
                                                    double* __restrict__ Dinv, double* __restrict__ Db) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= NX) return;
  const double* h6 = Hll + 6 * (size_t)l;
  const double m0 = h6[0] + lambda, m1 = h6[1], m2 = h6[2], m4 = h6[3] + lambda, m5 = h6[4], m8 = h6[5] + lambda;
  const double c00 = m4 * m8 - m5 * m5, c01 = m5 * m2 - m1 * m8, c02 = m1 * m5 - m4 * m2;
  const double det = m0 * c00 + m1 * c01 + m2 * c02;
  const double id = 1.0 / det;
  const double d0 = c00 * id, d1 = c01 * id, d2 = c02 * id, d3 = (m0 * m8 - m2 * m2) * id, d4 = (m2 * m1 - m0 * m5) * id,
               d5 = (m0 * m4 - m1 * m1) * id;
  double* o = Dinv + 6 * (size_t)l;
  o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3; o[4] = d4; o[5] = d5;
  const double* b = bl + 3 * (size_t)l;
  double* ob = Db + 3 * (size_t)l;
  ob[0] = d0 * b[0] + d1 * b[1] + d2 * b[2];
  ob[1] = d1 * b[0] + d3 * b[1] + d4 * b[2];
  ob[2] = d2 * b[0] + d4 * b[1] + d5 * b[2];
}

// The end of a workgroup's pass over the edges of free pose p, acc = each thread's Hpp (21 upper entries) | bp (6) over edges t,
// t + 256, ... of the pose's list: 27 wave sums, the four waves added in order, thread i stores entry i
__device__ __forceinline__ void schur_pose_tail(const double (&acc)[27], int p, double* __restrict__ Hpp, double* __restrict__ bp) {
  __shared__ double wpart[4][27];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 27; i++) {
    const double v = wave_sum_f64(acc[i]);
    if (lane == 0) wpart[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 27) {
    const double v = ((wpart[0][threadIdx.x] + wpart[1][threadIdx.x]) + wpart[2][threadIdx.x]) + wpart[3][threadIdx.x];
    if (threadIdx.x < 21) Hpp[21 * (size_t)p + threadIdx.x] = v;
    else bp[6 * (size_t)p + threadIdx.x - 21] = v;
  }
}

// Items [b, e) of a pose pair, thread t takes items t, t + 256, ... in order: sum_l Hpl_al Dinv_l Hpl_bl^T (6 x 6, entries 0 .. 35) and,
// on a diagonal pair, sum_l Hpl_al (Dinv_l bl_l) (entries 36 .. 41) as the four waves' sums in wpart, complete for every thread on
// return.  The caller adds them as ((w0 + w1) + w2) + w3.
template <int STRIDE>
__device__ __forceinline__ void schur_pair_items(bool diag, int b, int e, const SchurItem* __restrict__ items, const lba_edge* __restrict__ edges,
                                                 const double* __restrict__ EB, const double* __restrict__ Dinv, const double* __restrict__ Db,
                                                 double (*wpart)[42]) {
  double acc[42];
#pragma unroll
  for (int i = 0; i < 42; i++) acc[i] = 0;
  for (int q = b + threadIdx.x; q < e; q += 256) {
    const SchurItem it = items[q];
    const int l = edges[it.ea].point;
    const double* Ha = EB + (size_t)it.ea * STRIDE;
    const double* Hb = EB + (size_t)it.eb * STRIDE;
    const double* d = Dinv + 6 * (size_t)l;
    const double d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], d5 = d[5];
    double Wm[18];                                 // Hpl_a Dinv  (6 x 3)
#pragma unroll
    for (int a = 0; a < 6; a++) {
      const double h0 = Ha[3 * a], h1 = Ha[3 * a + 1], h2 = Ha[3 * a + 2];
      Wm[3 * a] = h0 * d0 + h1 * d1 + h2 * d2;
      Wm[3 * a + 1] = h0 * d1 + h1 * d3 + h2 * d4;
      Wm[3 * a + 2] = h0 * d2 + h1 * d4 + h2 * d5;
    }
    double hb[18];
#pragma unroll
    for (int i = 0; i < 18; i++) hb[i] = Hb[i];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c < 6; c++) acc[6 * a + c] += Wm[3 * a] * hb[3 * c] + Wm[3 * a + 1] * hb[3 * c + 1] + Wm[3 * a + 2] * hb[3 * c + 2];
    if (diag) {
      const double* db = Db + 3 * (size_t)l;
#pragma unroll
      for (int a = 0; a < 6; a++) acc[36 + a] += Ha[3 * a] * db[0] + Ha[3 * a + 1] * db[1] + Ha[3 * a + 2] * db[2];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 42; i++) {
    const double v = wave_sum_f64(acc[i]);
    if (lane == 0) wpart[wave][i] = v;
  }
  __syncthreads();
}

// Entry (r, cc) of the n x n reduced system and its mirror image, into the matrix-core solvers' tile image St or the dense S.  Every
// entry and its mirror are written by ONE thread, with one value: on a diagonal block the caller sends the thread of (a, c), a <= c,
// alone (the sum of (c, a) is the same number rounded otherwise).
__device__ __forceinline__ void schur_store_entry(int r, int cc, int n, double v, double* __restrict__ S, double* __restrict__ St) {
  if (St) {
    const int p0 = ldltm::tile_image_pos(r, cc), p1 = ldltm::tile_image_pos(cc, r);
    if (p0 >= 0) St[p0] = v;
    if (p1 >= 0 && r != cc) St[p1] = v;
  } else {
    S[(size_t)r * n + cc] = v;
    if (r != cc) S[(size_t)cc * n + r] = v;
  }
}

// Point l of a trial: x_l = Dinv_l (bl_l - sum Hpl_il^T x_i) over its edges in order (col_off(c): where free pose column c's six
// pose unknowns start in x), the trial estimate, and the point's term of computeScale: sum_j x_j (lambda x_j + b_j).  A point without
// edges, or a failed solve, keeps its estimate.
template <int STRIDE, class ColOff>
__device__ __forceinline__ void schur_update_point(int l, bool ok, const int* __restrict__ pose_col, ColOff col_off, const double* __restrict__ points,
                                                   const double* __restrict__ x, const int* __restrict__ pt_start, const int* __restrict__ pt_end,
                                                   const lba_edge* __restrict__ edges, const double* __restrict__ EB,
                                                   const double* __restrict__ Dinv, const double* __restrict__ bl, double lambda,
                                                   double* __restrict__ points_out, double* __restrict__ scale_out) {
  const int b = pt_start[l], e = pt_end[l];
  double sc = 0;
  double X[3] = {points[3 * (size_t)l], points[3 * (size_t)l + 1], points[3 * (size_t)l + 2]};
  if (e > b && ok) {
    double rr[3] = {bl[3 * (size_t)l], bl[3 * (size_t)l + 1], bl[3 * (size_t)l + 2]};
    for (int k = b; k < e; k++) {
      const int c = pose_col[edges[k].pose];
      if (c < 0) continue;
      const double* H = EB + (size_t)k * STRIDE;
      const double* xi = x + col_off(c);
#pragma unroll
      for (int cc = 0; cc < 3; cc++) {
        double s = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) s += H[3 * a + cc] * xi[a];
        rr[cc] -= s;
      }
    }
    const double* d = Dinv + 6 * (size_t)l;
    const double xl[3] = {d[0] * rr[0] + d[1] * rr[1] + d[2] * rr[2], d[1] * rr[0] + d[3] * rr[1] + d[4] * rr[2],
                          d[2] * rr[0] + d[4] * rr[1] + d[5] * rr[2]};
#pragma unroll
    for (int a = 0; a < 3; a++) { sc += xl[a] * (lambda * xl[a] + bl[3 * (size_t)l + a]); X[a] += xl[a]; }
  }
  points_out[3 * (size_t)l] = X[0]; points_out[3 * (size_t)l + 1] = X[1]; points_out[3 * (size_t)l + 2] = X[2];
  *scale_out = sc;
}

// The host's one pass over an edge list: indices in range, no edge of a kind the entry point does not take (is_right: the right camera
// of a rig), a point's observations consecutive (point never decreases), one observation per pose and point
template <class IsRight>
int schur_check_edges(const lba_edge* edges, int n_edges, int n_poses, int n_points, IsRight is_right) {
  std::vector<int> stamp((size_t)std::max(n_poses, 1), -1);
  int prev = -1;
  for (int k = 0; k < n_edges; k++) {
    const lba_edge& e = edges[k];
    if (e.pose < 0 || e.pose >= n_poses || e.point < 0 || e.point >= n_points) return ORBG_BAD_ARG;
    if (is_right(e.ur)) return ORBG_BAD_ARG;
    if (e.point < prev) return ORBG_BAD_ARG;                      // per point, its observations
    if (stamp[e.pose] == e.point) return ORBG_BAD_ARG;            // one observation per pose and point
    stamp[e.pose] = e.point;
    prev = e.point;
  }
  return ORBG_OK;
}
