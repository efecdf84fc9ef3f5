// orbgpu_inertial.hpp over the mock types of mock_inertial.hpp: builds a Frame from the numbers in a text file, calls the glue and dumps
// what it handed over (--cpu: the library call is replaced by one that records the problem and returns a canned result) and what it
// wrote back (both modes; --gpu runs the real call).  tests/test_pose_inertial_glue.py writes the file and reads the dump.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mock_inertial.hpp"
#include "orbgpu_inertial.hpp"

using namespace mock;

static FILE* g_in;
static double rd() { double x; if (fscanf(g_in, "%lf", &x) != 1) { fprintf(stderr, "short input\n"); exit(2); } return x; }
static void rd_mat(Mat& m) { for (float& x : m.d) x = (float)rd(); }
static void dump_f(const char* name, const float* p, size_t n) { printf("%s", name); for (size_t i = 0; i < n; i++) printf(" %.9g", (double)p[i]); printf("\n"); }
static void dump_d(const char* name, const double* p, size_t n) { printf("%s", name); for (size_t i = 0; i < n; i++) printf(" %.17g", p[i]); printf("\n"); }

struct RecordOps {
  static int information(const float* C, double* i9, double* ig, double* ia) { dump_f("C", C, 225); return orbg_imu_information(C, i9, ig, ia); }
  static int optimize(const pose_inertial_problem& p, pose_inertial_result& r) {
    const double head[6] = {(double)p.struct_size, (double)p.form, (double)p.rec_init, (double)p.device, (double)p.n_left, (double)p.n};
    dump_d("head", head, 6);
    dump_f("Xw", p.Xw, 3 * (size_t)p.n); dump_f("u", p.u, p.n); dump_f("v", p.v, p.n); dump_f("ur", p.ur, p.n); dump_f("inv_sigma2", p.inv_sigma2, p.n);
    printf("close"); for (int i = 0; i < p.n; i++) printf(" %d", p.close[i]); printf("\n");
    const float cam[5] = {p.fx, p.fy, p.cx, p.cy, p.bf};
    dump_f("cam", cam, 5); dump_f("Tcb", p.Tcb, 12);
    dump_f("frame", p.frame.Rwb, 21); dump_f("other", p.other.Rwb, 21);
    dump_f("preint", &p.preint.dT, sizeof(p.preint) / sizeof(float));
    dump_d("info9", p.info9, 81); dump_d("infoG", p.infoG, 9); dump_d("infoA", p.infoA, 9);
    if (p.prior) dump_d("prior", p.prior->Rwb, sizeof(*p.prior) / sizeof(double));
    // a canned result
    for (int i = 0; i < 9; i++) r.Rwb[i] = 0.125 * i + 1e-9;
    for (int i = 0; i < 3; i++) { r.twb[i] = 10.0 + i + 1e-9; r.vwb[i] = 20.0 + i; r.bg[i] = 0.5 + i; r.ba[i] = -0.5 - i; }
    for (int i = 0; i < 225; i++) r.H[i] = i + 1;
    for (int i = 0; i < p.n; i++) r.outlier[i] = i % 3 == 0;
    r.n_inliers = 77; r.n_bad = p.n - 77; r.rounds_run = 4;
    return ORBG_OK;
  }
};

struct MockFactory {
  template <class CpiT>
  static CpiT* make(const pose_inertial_result& r) {
    CpiT* c = new CpiT();
    for (int i = 0; i < 9; i++) c->Rwb.v[i] = r.Rwb[i];
    for (int i = 0; i < 3; i++) { c->twb.v[i] = r.twb[i]; c->vwb.v[i] = r.vwb[i]; c->bg.v[i] = r.bg[i]; c->ba.v[i] = r.ba[i]; }
    for (int i = 0; i < 225; i++) c->H.v[i] = r.H[i];
    orbg_condition_prior(c->H.v);                        // what the reference's constructor does (I/G2oTypes.h:712-718)
    return c;
  }
};

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s --cpu|--gpu input.txt\n", argv[0]); return 2; }
  const bool gpu = std::string(argv[1]) == "--gpu";
  g_in = fopen(argv[2], "r");
  if (!g_in) return 2;
  const int form = (int)rd(), rec_init = (int)rd(), N = (int)rd(), two_cam = (int)rd(), no_cpi = (int)rd();
  Frame F, Fp; KeyFrame K; Preintegrated I;
  F.N = N; F.mvpMapPoints.assign(N, nullptr); F.mvbOutlier.assign(N, true); F.mvKeysUn.resize(N); F.mvuRight.resize(N);
  std::vector<MapPoint*> owned;
  for (int i = 0; i < N; i++) {
    const int has = (int)rd();
    float X[3] = {(float)rd(), (float)rd(), (float)rd()};
    F.mvKeysUn[i].pt.x = (float)rd(); F.mvKeysUn[i].pt.y = (float)rd(); F.mvKeysUn[i].octave = (int)rd();
    F.mvuRight[i] = (float)rd();
    const float depth = (float)rd();
    if (has) { owned.push_back(new MapPoint(X)); owned.back()->mTrackDepth = depth; F.mvpMapPoints[i] = owned.back(); }
  }
  F.mvInvLevelSigma2.resize(8);
  for (float& x : F.mvInvLevelSigma2) x = (float)rd();
  F.fx = (float)rd(); F.fy = (float)rd(); F.cx = (float)rd(); F.cy = (float)rd(); F.mbf = (float)rd();
  rd_mat(F.mImuCalib.Tcb);
  auto rd_state = [&](Mat& R, Mat& t, Mat& v, Bias& b) {
    rd_mat(R); rd_mat(t); rd_mat(v);
    b.bwx = (float)rd(); b.bwy = (float)rd(); b.bwz = (float)rd(); b.bax = (float)rd(); b.bay = (float)rd(); b.baz = (float)rd();
  };
  Mat R(3, 3), t(3, 1), v(3, 1); Bias b;
  rd_state(R, t, v, b);
  F.SetImuPoseVelocity(R, t, v); F.mImuBias = b; F.set_calls = 0;
  rd_state(R, t, v, b);
  Fp.SetImuPoseVelocity(R, t, v); Fp.mImuBias = b;
  Mat bg(3, 1), ba(3, 1);
  bg.d = {b.bwx, b.bwy, b.bwz}; ba.d = {b.bax, b.bay, b.baz};
  K.set(R, t, v, bg, ba);
  I.dT = (float)rd();
  rd_mat(I.dR); rd_mat(I.dV); rd_mat(I.dP); rd_mat(I.JRg); rd_mat(I.JVg); rd_mat(I.JVa); rd_mat(I.JPg); rd_mat(I.JPa);
  I.b.bwx = (float)rd(); I.b.bwy = (float)rd(); I.b.bwz = (float)rd(); I.b.bax = (float)rd(); I.b.bay = (float)rd(); I.b.baz = (float)rd();
  rd_mat(I.C);
  if (form == POSE_INERTIAL_LAST_FRAME) {
    F.mpImuPreintegratedFrame = &I; F.mpPrevFrame = &Fp;
    if (!no_cpi) {
      Fp.mpcpi = new ConstraintPoseImu();
      for (double& x : Fp.mpcpi->Rwb.v) x = rd();
      for (double& x : Fp.mpcpi->twb.v) x = rd();
      for (double& x : Fp.mpcpi->vwb.v) x = rd();
      for (double& x : Fp.mpcpi->bg.v) x = rd();
      for (double& x : Fp.mpcpi->ba.v) x = rd();
      for (double& x : Fp.mpcpi->H.v) x = rd();
    }
  } else {
    F.mpImuPreintegrated = &I; F.mpLastKeyFrame = &K;
  }
  if (two_cam) F.Nleft = N / 2;
  int ret = 0;
  try {
    if (form == POSE_INERTIAL_LAST_FRAME)
      ret = gpu ? orbgpu::PoseInertialOptimizationLastFrame<orbgpu::inertial::GpuOps, MockFactory>(&F, rec_init != 0)
                : orbgpu::PoseInertialOptimizationLastFrame<RecordOps, MockFactory>(&F, rec_init != 0);
    else
      ret = gpu ? orbgpu::PoseInertialOptimizationLastKeyFrame<orbgpu::inertial::GpuOps, MockFactory>(&F, rec_init != 0)
                : orbgpu::PoseInertialOptimizationLastKeyFrame<RecordOps, MockFactory>(&F, rec_init != 0);
  } catch (const std::exception& e) {
    printf("threw %s\n", e.what());
    return 0;
  }
  printf("ret %d\n", ret);
  printf("mvbOutlier"); for (int i = 0; i < N; i++) printf(" %d", (int)F.mvbOutlier[i]); printf("\n");
  const Mat oR = F.GetImuRotation(), ot = F.GetImuPosition();
  dump_f("Rwb", oR.d.data(), 9); dump_f("twb", ot.d.data(), 3); dump_f("Vw", F.mVw.d.data(), 3);
  const float bias[6] = {F.mImuBias.bwx, F.mImuBias.bwy, F.mImuBias.bwz, F.mImuBias.bax, F.mImuBias.bay, F.mImuBias.baz};
  dump_f("bias_g_a", bias, 6);
  dump_d("cpi", F.mpcpi->Rwb.v, 9); dump_d("cpi_t", F.mpcpi->twb.v, 3); dump_d("cpi_v", F.mpcpi->vwb.v, 3); dump_d("cpi_bg", F.mpcpi->bg.v, 3);
  dump_d("cpi_ba", F.mpcpi->ba.v, 3); dump_d("cpi_H", F.mpcpi->H.v, 225);
  printf("prev_cpi_null %d\nlive %d\nset_calls %d\n", Fp.mpcpi == nullptr, ConstraintPoseImu::live, F.set_calls);
  return 0;
}
