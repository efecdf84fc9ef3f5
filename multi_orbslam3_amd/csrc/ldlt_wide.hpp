// The many-workgroup LDL^T of reduced camera systems beyond the matrix-core kernels (ldlt_mfma.hpp, ldlt_xcd.hpp), used by the
// local BA (lba.hip) and the full BA (full_ba.hip).  No include guard and no namespace of its own: each translation unit
// includes it ONCE inside its anonymous namespace.

// ---- Blocked LDL^T + solve over MANY workgroups, for windows beyond the matrix-core kernels (more than 50 free poses:
// the matrix-core kernels hold <= 19 tile rows in one CU's registers, the row-pair kernel <= 1344 blocks).  Right-looking,
// 16-column blocks, dense row-major S in global memory (L2-resident), two launches per block column:
//   k_wide_panel(kb):  every workgroup factors the 16 x 16 diagonal block itself (no hand-over between workgroups).  The
//                      block is READ from its diagonal and upper triangle only and workgroup 0 WRITES the strictly lower
//                      triangle only (L_kk for the back-substitution), so a workgroup that is dispatched after workgroup 0
//                      has finished still factors the unfactored block: no location is input and output of one launch;
//                      workgroup 0 also forward-substitutes the right-hand side's block, workgroup g >= 1 turns
//                      row block kb + g into L = A L_kk^-T D^-1 (in place) and W = L D (kept in the mirrored upper block);
//   k_wide_update(kb): A_ij -= W_ik L_jk^T for every trailing block, and the right-hand side as one more row;
// then k_wide_back: x = L^-T z in one workgroup.  Same failure rule as k_ldlt: a zero / non-finite pivot clears the flag.
__global__ __launch_bounds__(256) void k_wide_panel(int n, int kb, double* S, const double* __restrict__ b, double* yw, double* z,
                                                    int* __restrict__ ok_flag) {
  __shared__ double Lk[16][17];
  __shared__ double Aw[16][17];
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
  const int k0 = 16 * kb;
  {
    const int gr = k0 + r, gc = k0 + c;
    const int lo = gr < gc ? gr : gc, hi = gr < gc ? gc : gr;
    Lk[r][c] = (gr < n && gc < n) ? S[(size_t)lo * n + hi] : (r == c ? 1.0 : 0.0);
  }
  if (blockIdx.x == 0 && kb == 0 && tid == 0) *ok_flag = 1;
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < 16; j++) {
    const double d = Lk[j][j];
    if (d == 0.0 || !(d == d) || fabs(d) == INFINITY) bad = true;
    const bool below = r > j, upd = below && c > j && c <= r;
    double v = 0.0, wc = 0.0;
    if (below) v = Lk[r][j];
    if (upd) wc = Lk[c][j];
    __syncthreads();
    const double l = v / d;
    if (upd) Lk[r][c] -= l * wc;
    if (below && c == j) Lk[r][j] = l;
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    if (bad && tid == 0) *ok_flag = 0;
    const int gr = k0 + r, gc = k0 + c;
    if (gr < n && gc < n && c < r) S[(size_t)gr * n + gc] = Lk[r][c];
    // the right-hand side as a one-row block: w = b_k^T L_kk^-T (kept for the trailing update), z = w / D
    const double* src = kb == 0 ? b : yw;
    Aw[r][c] = (r == 0 && k0 + c < n) ? src[k0 + c] : 0.0;
    __syncthreads();
    for (int m = 0; m < 15; m++) {
      if (r == 0 && c > m) Aw[0][c] -= Aw[0][m] * Lk[c][m];
      __syncthreads();
    }
    if (r == 0 && k0 + c < n) { const double w = Aw[0][c]; yw[k0 + c] = w; z[k0 + c] = w / Lk[c][c]; }
    return;
  }
  const int i0 = 16 * (kb + (int)blockIdx.x);
  Aw[r][c] = i0 + r < n ? S[(size_t)(i0 + r) * n + k0 + c] : 0.0;
  __syncthreads();
  for (int m = 0; m < 15; m++) {
    if (c > m) Aw[r][c] -= Aw[r][m] * Lk[c][m];
    __syncthreads();
  }
  if (i0 + r < n) {
    const double w = Aw[r][c];
    S[(size_t)(i0 + r) * n + k0 + c] = w / Lk[c][c];
    S[(size_t)(k0 + c) * n + i0 + r] = w;
  }
}

// grid (m, m + 1), m = trailing row blocks: block (jj, ii) updates tile (kb+1+ii, kb+1+jj), ii >= jj; row ii == m is the right-hand side
__global__ __launch_bounds__(256) void k_wide_update(int n, int kb, double* S, const double* __restrict__ b, double* yw) {
  const int m_blocks = gridDim.x, jj = blockIdx.x, ii = blockIdx.y;
  if (ii < m_blocks && ii < jj) return;
  __shared__ double Wt[16][17];
  __shared__ double Lj[16][17];
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
  const int k0 = 16 * kb, j0 = 16 * (kb + 1 + jj);
  Lj[r][c] = j0 + r < n ? S[(size_t)(j0 + r) * n + k0 + c] : 0.0;               // L_jk[r][c]
  if (ii == m_blocks) {
    if (r == 0) Wt[0][c] = yw[k0 + c];
    __syncthreads();
    if (r == 0 && j0 + c < n) {
      double acc = 0.0;
      for (int m = 0; m < 16; m++) acc += Wt[0][m] * Lj[c][m];
      yw[j0 + c] = (kb == 0 ? b[j0 + c] : yw[j0 + c]) - acc;
    }
    return;
  }
  const int i0 = 16 * (kb + 1 + ii);
  Wt[c][r] = i0 + c < n ? S[(size_t)(k0 + r) * n + i0 + c] : 0.0;               // W_ik[c][r], read along the mirrored block's rows
  __syncthreads();
  if (i0 + r < n && j0 + c < n) {
    double acc = 0.0;
    for (int m = 0; m < 16; m++) acc += Wt[r][m] * Lj[c][m];
    S[(size_t)(i0 + r) * n + j0 + c] -= acc;
  }
}

__global__ __launch_bounds__(1024) void k_wide_back(int n, const double* __restrict__ S, const double* __restrict__ z, double* __restrict__ x,
                                                    const int* __restrict__ ok_flag) {
  extern __shared__ double xs[];
  if (*ok_flag == 0) return;
  const int tid = threadIdx.x, T = (n + 15) / 16;
  for (int i = tid; i < n; i += 1024) xs[i] = z[i];
  __syncthreads();
  for (int kb = T - 1; kb >= 0; kb--) {
    const int k0 = 16 * kb, w = min(16, n - k0);
    if (tid < 64) {
      // the diagonal block: lane i < 16 holds x_i and column i of L_kk; x_j goes round by a lane read, 15 steps in registers
      const int i = tid & 15;
      double lcol[16];
#pragma unroll
      for (int j = 0; j < 16; j++) lcol[j] = (j > i && j < w) ? S[(size_t)(k0 + j) * n + k0 + i] : 0.0;
      double xv = i < w ? xs[k0 + i] : 0.0;
#pragma unroll
      for (int j = 15; j > 0; j--) {
        const double xj = __shfl(xv, j, 16);
        xv -= lcol[j] * xj;
      }
      if (tid < w) xs[k0 + tid] = xv;
    }
    __syncthreads();
    for (int i = tid; i < k0; i += 1024) {
      double acc = 0.0;
      for (int cc = 0; cc < w; cc++) acc += S[(size_t)(k0 + cc) * n + i] * xs[k0 + cc];
      xs[i] -= acc;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += 1024) x[i] = xs[i];
}

constexpr int kWideMaxUnknowns = 8192;   // k_wide_back keeps x in LDS: n * 8 bytes <= 64 KB (1365 free poses)
static hipError_t launch_ldlt_wide(int n, double* S, const double* b, double* x, int* ok, double* scratch, hipStream_t st) {
  if (n > kWideMaxUnknowns) return hipErrorInvalidValue;
  const int T = (n + 15) / 16;
  double* yw = scratch;
  double* z = scratch + n;
  for (int kb = 0; kb < T; kb++) {
    hipLaunchKernelGGL(k_wide_panel, dim3(T - kb), dim3(256), 0, st, n, kb, S, b, yw, z, ok);
    const int m = T - kb - 1;
    if (m > 0) hipLaunchKernelGGL(k_wide_update, dim3(m, m + 1), dim3(256), 0, st, n, kb, S, b, yw);
  }
  hipLaunchKernelGGL(k_wide_back, dim3(1), dim3(1024), (size_t)n * sizeof(double), st, n, S, z, x, ok);
  return hipGetLastError();
}
