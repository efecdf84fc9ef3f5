// The host side of the dense LDL^T that ends an LM trial of the local BA (lba.hip), the full and the welding BA (full_ba.hip) and
// the essential graph (essential_graph.hip): the two switches, the choice of a kernel family by size, its buffers, the launch and
// the way back from a timed-out eight-workgroup launch.  No include guard and no namespace of its own: each translation unit
// includes it ONCE inside its anonymous namespace, after ldlt_mfma.hpp, ldlt_xcd.hpp and ldlt_wide.hpp.

// an attempt's return code when k_ldlt_xcd reported kOkTimedOut (never leaves the library: ldlt_retry answers it)
constexpr int kRcLdltTimedOut = -70001;

// The switches are read ONCE per owner (lba_create, ba_create, a thread's first eg_solve) -- no solve path calls getenv:
// ORBG_LDLT_WIDE=1 sends every size to the many-workgroup blocked LDL^T (k_wide_*: the solver beyond ldlt_mfma.hpp's sizes) so that
// tests can run it on small problems.  ORBG_LDLT_XCD=0 keeps the sizes of the eight-workgroup kernel (ldlt_xcd.hpp) on the
// one-workgroup kernels; =safe forces that kernel's agent-scope hand-overs (the path it takes by itself when its workgroups do not
// share an XCD); =short is the local BA's test hook (asked_short: lba.hip hands it to launch() once, nobody else looks at it).
struct LdltSolver {
  bool wide = false;
  int xcd = 1;                         // 0 off, 1 on, 2 on with forced safe hand-overs
  bool asked_short = false;
  bool env_read = false;
  bool keep_dense = false;             // the owner's assembly writes the dense S on every path (the local BA's k_schur)
  int n = 0;                           // what plan() planned for; 0: nothing to solve
  bool use_mfma = false, use_xcd = false;
  ldltm::AttrCache attr;               // which kernels of the owner's device already allow their dynamic LDS size
  ldltx::Context x;                    // flags / scratch / launch counter of the eight-workgroup LDL^T
  DevBuf<double> d_S, d_St, d_wfac;    // the system dense / as a tile image, factor scratch of the one-workgroup kernels
  DevBuf<double> d_wide;               // running / scaled right-hand side of k_wide_*
  DevBuf<double> d_xscr; DevBuf<unsigned> d_xflags;

  void read_env() {
    if (env_read) return;
    wide = getenv("ORBG_LDLT_WIDE") != nullptr;
    if (const char* e = getenv("ORBG_LDLT_XCD")) { xcd = !strcmp(e, "0") ? 0 : !strcmp(e, "safe") ? 2 : 1; asked_short = !strcmp(e, "short"); }
    env_read = true;
  }

  // the kernel family for n_ unknowns, its buffers, and on first use the eight-workgroup context
  int plan(int n_, hipStream_t st) {
    int rc;
    n = n_;
    use_mfma = n >= 1 && ldltm::supports(n) && !wide;
    const bool use_wide = n >= 1 && !use_mfma;
    if (use_wide && n > kWideMaxUnknowns) return ORBG_CAP_EXCEEDED;      // (k_wide_back's x lives in LDS)
    if (use_wide && (rc = d_wide.reserve(2 * (size_t)n + 32))) return rc;
    if ((use_wide || keep_dense) && (rc = d_S.reserve(std::max<size_t>((size_t)n * n, 1)))) return rc;
    if (use_mfma && ((rc = d_St.reserve(ldltm::tile_image_doubles(n))) || (rc = d_wfac.reserve(ldltm::wglob_doubles(ldltm::make_geo(n))))))
      return rc;
    use_xcd = use_mfma && xcd != 0 && ldltx::pays(n);
    if (use_xcd && !x.scr) {
      if ((rc = d_xscr.reserve(ldltx::scratch_doubles())) || (rc = d_xflags.reserve(ldltx::kFlagWords))) return rc;
      ORBG_HIP(hipMemsetAsync(d_xflags.p, 0, ldltx::kFlagWords * sizeof(unsigned), st));
      // (the G / D^-1 pair region: a fresh nonce per bind already makes stale pairs of a recycled allocation fail their test; zero all the same)
      ORBG_HIP(hipMemsetAsync(d_xscr.p + ldltx::kGbOff, 0, (ldltx::kWOff - ldltx::kGbOff) * sizeof(double), st));
      x.bind(d_xscr.p, d_xflags.p);
      x.pick = ((int)getpid() + next_ldlt_xcd_user()) & 7;   // users of one process on different XCDs; processes sharing a GPU differ by pid
    }
    return ORBG_OK;
  }

  // what the assembly kernels write: the tile image or the dense matrix, NULL for the one this size does not use
  double* St() const { return use_mfma ? d_St.p : nullptr; }
  double* S() const { return use_mfma && !keep_dense ? nullptr : d_S.p; }

  // absent blocks: ONE fill of the system (the tile image's padding and border follow, they do not depend on the values), and the
  // zeroed solution
  int clear(double* xv, hipStream_t st) {
    if (use_mfma) {
      ORBG_HIP(hipMemsetAsync(d_St.p, 0, sizeof(double) * ldltm::tile_image_doubles(n), st));
      ORBG_HIP(ldltm::launch_image_pad(n, d_St.p, st));
    } else {
      ORBG_HIP(hipMemsetAsync(d_S.p, 0, sizeof(double) * (size_t)n * n, st));
    }
    ORBG_HIP(hipMemsetAsync(xv, 0, sizeof(double) * (size_t)n, st));
    return ORBG_OK;
  }

  // factor and solve: x, and *ok (0: a pivot failed, ldltx::kOkTimedOut: see timed_out)
  int launch(const double* b, double* xv, int* ok, hipStream_t st, bool one_short = false) {
    if (use_xcd) ORBG_HIP(ldltx::launch(x, n, d_St.p, xv, ok, st, ldltx::kMaxP, xcd == 2, one_short));
    else if (use_mfma) ORBG_HIP(ldltm::launch(n, d_St.p, xv, ok, d_wfac.p, st, &attr));
    else ORBG_HIP(launch_ldlt_wide(n, d_S.p, b, xv, ok, d_wide.p, st));
    return ORBG_OK;
  }

  // A launch of the eight-workgroup LDL^T whose participants were not all placed in time says so instead of posing as a
  // non-positive-definite system, which an LM loop would answer with a rejected step and another trajectory than the reference's.
  static bool timed_out(int ok_value) { return ok_value == ldltx::kOkTimedOut; }
  void drop_xcd() { xcd = 0; }

  void release() {
    for (DevBuf<double>* b : {&d_S, &d_St, &d_wfac, &d_wide, &d_xscr}) b->release();
    d_xflags.release();
    x.scr = nullptr; x.flags = nullptr;
  }
};

// what a solve's timed_out() (lm_optimize, lm_driver.hpp) answers from the flag of its last record
inline int ldlt_timed_out_rc(int ok_value) { return LdltSolver::timed_out(ok_value) ? kRcLdltTimedOut : ORBG_OK; }

// Runs `attempt` (a whole solve from the caller's untouched input).  A time-out is not a verdict on the system: the owner of `s`
// stops using the eight-workgroup kernel -- the ORBG_LDLT_XCD=0 path, parity-tested like the default -- and the attempt runs once more.
template <class Attempt>
int ldlt_retry(LdltSolver& s, hipStream_t st, Attempt attempt, bool* retried = nullptr) {
  int rc = attempt();
  if (retried) *retried = rc == kRcLdltTimedOut;
  if (rc != kRcLdltTimedOut) return rc;
  s.drop_xcd();
  if (hipStreamSynchronize(st) != hipSuccess) return ORBG_HIP_ERROR;
  rc = attempt();
  return rc == kRcLdltTimedOut ? ORBG_HIP_ERROR : rc;
}
