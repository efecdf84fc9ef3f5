// ORBmatcher::Fuse (S/ORBmatcher.cc:1395-1605, the LocalMapping overload with bRight = false, and :1607-1742, the Sim3 overload of
// LoopClosing::SearchAndFuse) for gfx950: every (target keyframe k, map point i) pair of a call in ONE kernel launch, one record per
// pair at [k * P + i], then the reference's serial bookkeeping replayed on the host over the records
// (include/orbgpu_localmapping.hpp).
//
// Why one launch is enough.  For one pair everything up to bestIdx / bestDist reads the keyframe's pose, intrinsics, keypoints,
// mvuRight, grid and descriptors and the point's position, normal, distance range and descriptor.  During
// LocalMapping::SearchInNeighbors (S/LocalMapping.cc:868-976) none of these changes except the descriptor (MapPoint::Replace ends in
// ComputeDistinctiveDescriptors on the survivor, S/MapPoint.cc:367-419).  The set of candidates that pass the level and chi2 gates
// does not depend on the descriptor, so the record carries it (the first ORBG_FUSE_CAND_CAP = 16 indices in vIndices order and the
// exact count): the host rescores a pair whose point has a new descriptor over that list, first strict minimum wins.  isBad(),
// IsInKeyFrame(), GetMapPoint(bestIdx) and Observations() are host state and stay with the replay.
//
// Shape.  On the scenes of tests/fuse_model.py, where every target looks at what the current keyframe sees, four pairs in ten end at
// a frustum gate, three more find an empty window and three reach the candidate loop; second neighbours of a real map share less
// with the current keyframe.  A wavefront per pair -- the shape of the Tracking searches in matcher.hip -- would idle 63 lanes for
// most of the grid.  Grid = (ceil(P / 256), K), a workgroup is 4 wavefronts:
//   Gates    one LANE per pair: depth, image, distance range, normal, PredictScale and the cell window of GetFeaturesInArea with
//            its four early returns.  A pair that ends here writes its record and an all-0xFFFF candidate list and is done; a
//            survivor leaves (u, v, ur, r, level, window) in LDS (28 B per pair, 7 KB per workgroup: no limit on occupancy, the
//            kernel needs no other LDS) and takes a slot of the workgroup's survivor list by ballot rank (no atomics).
//   Window   the 16 groups of 16 lanes take the survivors in turn, as newpoints.hip does for its buckets.  A window is 2 x 2 to
//            4 x 4 cells of ~10 features in all: the lanes of a group take the cells in GetFeaturesInArea's order (ix outer, iy
//            inner), 16 cells per step.  Pass 1 counts per lane the features inside the window and those that pass the level / chi2
//            gates; an inclusive scan over the 16 lanes turns the counts into each lane's first rank in vIndices order.  Pass 2
//            walks the same cells again (L2 / L1 hits), writes the candidates of rank < 16 straight to the list and keeps
//            min(dist << 40 | rank << 16 | idx): smallest distance, earliest rank -- the reference's strict `dist < bestDist`.
//            A 4-step xor butterfly gives the group's winner; lane 0 writes the record, lanes >= n_cand pad the list with 0xFFFF.
// 72 VGPRs, no scratch, 7 KB of LDS: seven wavefronts per SIMD, so the dependent loads of the window walk (cell -> item -> keypoint ->
// descriptor) of one group hide behind the other wavefronts'.  No atomics, every reduction is an integer min or sum: two runs give
// the same bits.
//
// Arithmetic: the choices of this code path, not new ones.
//   search_sim3_kernel (matcher.hip): p3Dc = Rcw p3Dw + tcw in float, k order (pose_map); cv::norm(PO) with double accumulation,
//   rounded to float (norm3d); PO.dot(Pn) in double against 0.5 * dist3D; PredictScale as (float)log((double)ratio) / mfLogScaleFactor
//   on the raw mfMaxDistance, ceilf, clamped; the 1.2f / 0.8f invariance factors of S/MapPoint.cc:617-627.
//   N-1 / N-9 of newpoints.hip: Pinhole::project is fx * x / z + cx in float, left to right; a float compared with a double literal
//   is promoted: (double)(e2 * mvInvLevelSigma2[kpLevel]) > 7.8 | 5.99 (:1540, :1551).  invz = 1 / z and ur = u - bf * invz are float.
// Built with -ffp-contract=off and correctly rounded float divide / sqrt, like the rest of the library.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "grid_build.hpp"

using orbg::FrameParams;

// matcher.hip
int orbm_internal_kf_features(orbm_frame* f, const orbx_keypoint** d_kps, const uint8_t** d_desc, const float** d_uright,
                              const float** d_depth, const orbx_keypoint** h_kps, int* n, int* device, hipStream_t* stream);
int orbm_internal_kf_grid(orbm_frame* f, const int** d_cell_start, const int** d_cell_items, FrameParams* fp);

namespace {

constexpr int kLanes = 16;          // lanes per surviving pair
constexpr int kThreads = 256;
constexpr int kGroups = kThreads / kLanes;
constexpr int kCap = ORBG_FUSE_CAND_CAP;
static_assert(kCap == kLanes, "the list is padded by one lane per slot");

struct FuseKfDev {                  // one target keyframe as the kernel reads it
  const orbx_keypoint* kps;         // mvKeysUn
  const uint8_t* desc;
  const float* uright;              // NULL: mvuRight = -1 throughout
  const int* cell_start; const int* cell_items;   // mGrid as CSR, cell = ix * 48 + iy, ascending feature index inside a cell
  float R[9], t[3], Ow[3];
  float fx, fy, cx, cy, bf;
  float min_x, max_x, min_y, max_y, w_inv, h_inv;
  float log_sf;
  int n_levels;
  float sf[ORBG_MAX_LEVELS], inv_sigma2[ORBG_MAX_LEVELS];
};

struct FuseArgs {
  const FuseKfDev* kf;              // K
  const float* pos; const float* normal; const float* min_dist; const float* max_dist;   // P
  const uint8_t* desc;              // P x 32
  const uint8_t* pskip;             // P, or NULL: bad | skip of the points view
  const uint8_t* skip;              // K x P, or NULL
  orbm_fuse_record* rec;            // K x P
  uint16_t* cand;                   // K x P x kCap
  int P;
  float th;
};

struct Survivor { float u, v, ur, r; int level; int cells; int local; };   // cells: minX | maxX << 8 | minY << 16 | maxY << 24

__device__ __forceinline__ int popc256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ int clamp_level(int o) { return o < 0 ? 0 : (o >= ORBG_MAX_LEVELS ? ORBG_MAX_LEVELS - 1 : o); }

// is feature idx inside the window (GetFeaturesInArea, S/KeyFrame.cc:926-935), and does it pass the per-candidate gates
// (S/ORBmatcher.cc:1526-1553 | :1703-1704)?
template <bool kSim3>
__device__ __forceinline__ void classify(const FuseKfDev& K, const Survivor& s, int idx, bool* in_window, bool* is_cand) {
  const orbx_keypoint kp = K.kps[idx];
  const float distx = kp.x - s.u, disty = kp.y - s.v;
  *in_window = fabsf(distx) < s.r && fabsf(disty) < s.r;
  *is_cand = false;
  if (!*in_window) return;
  const int kpLevel = kp.octave;
  if (kpLevel < s.level - 1 || kpLevel > s.level) return;
  if constexpr (!kSim3) {
    const float kpr = K.uright ? K.uright[idx] : -1.f;
    const float ex = s.u - kp.x, ey = s.v - kp.y;
    const float w = K.inv_sigma2[clamp_level(kpLevel)];
    if (kpr >= 0) {
      const float er = s.ur - kpr;
      const float e2 = ex * ex + ey * ey + er * er;
      if ((double)(e2 * w) > 7.8) return;
    } else {
      const float e2 = ex * ex + ey * ey;
      if ((double)(e2 * w) > 5.99) return;
    }
  }
  *is_cand = true;
}

__device__ __forceinline__ int group_incl_scan(int v, int sub) {
#pragma unroll
  for (int d = 1; d < kLanes; d <<= 1) {
    const int o = __shfl_up(v, d, kLanes);
    if (sub >= d) v += o;
  }
  return v;
}

template <bool kSim3>
__global__ __launch_bounds__(kThreads) void fuse_kernel(FuseArgs A) {
  __shared__ Survivor s_surv[kThreads];
  __shared__ int s_wcnt[kThreads / 64];
  const int k = blockIdx.y;
  const FuseKfDev& K = A.kf[k];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kInitDist = kSim3 ? INT_MAX : 256;

  // ---- gates: one lane per pair
  bool survives = false;
  Survivor sv;
  sv.u = sv.v = sv.ur = sv.r = 0.f; sv.level = -1; sv.cells = 0; sv.local = threadIdx.x;
  if (i < A.P) {
    int status = ORBM_FUSE_SKIPPED;
    if (!((A.pskip && A.pskip[i]) || (A.skip && A.skip[(size_t)k * A.P + i]))) {
      const float X[3] = {A.pos[3 * i], A.pos[3 * i + 1], A.pos[3 * i + 2]};
      float Pc[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float t0 = K.R[3 * a] * X[0] + K.R[3 * a + 1] * X[1] + K.R[3 * a + 2] * X[2];
        Pc[a] = t0 + K.t[a];
      }
      status = ORBM_FUSE_NEG_DEPTH;
      if (!(Pc[2] < 0.0f)) {                                                             // :1455
        const float invz = 1.0f / Pc[2];
        const float u = K.fx * Pc[0] / Pc[2] + K.cx, v = K.fy * Pc[1] / Pc[2] + K.cy;    // Pinhole::project
        status = ORBM_FUSE_NOT_IN_IMAGE;
        if (u >= K.min_x && u < K.max_x && v >= K.min_y && v < K.max_y) {               // KeyFrame::IsInImage
          const float max_raw = A.max_dist[i];
          const float maxDistance = 1.2f * max_raw, minDistance = 0.8f * A.min_dist[i];
          const float PO[3] = {X[0] - K.Ow[0], X[1] - K.Ow[1], X[2] - K.Ow[2]};
          const float dist3D = (float)sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
          status = ORBM_FUSE_DISTANCE;
          if (!(dist3D < minDistance || dist3D > maxDistance)) {                         // :1483
            const double dot = (double)PO[0] * A.normal[3 * i] + (double)PO[1] * A.normal[3 * i + 1] + (double)PO[2] * A.normal[3 * i + 2];
            status = ORBM_FUSE_NORMAL;
            if (!(dot < 0.5 * (double)dist3D)) {                                         // :1492
              const float ratio = max_raw / dist3D;                                      // MapPoint::PredictScale, S/MapPoint.cc:629-644
              const float lg = (float)log((double)ratio);
              int lvl = (int)ceilf(lg / K.log_sf);
              if (lvl < 0) lvl = 0;
              else if (lvl >= K.n_levels) lvl = K.n_levels - 1;
              const float r = A.th * K.sf[lvl];
              sv.u = u; sv.v = v; sv.ur = u - K.bf * invz; sv.r = r; sv.level = lvl;
              // KeyFrame::GetFeaturesInArea, S/KeyFrame.cc:898-912
              status = ORBM_FUSE_EMPTY_WINDOW;
              const int nMinCellX = max(0, (int)floorf((u - K.min_x - r) * K.w_inv));
              if (nMinCellX < ORBG_GRID_COLS) {
                const int nMaxCellX = min(ORBG_GRID_COLS - 1, (int)ceilf((u - K.min_x + r) * K.w_inv));
                if (nMaxCellX >= 0) {
                  const int nMinCellY = max(0, (int)floorf((v - K.min_y - r) * K.h_inv));
                  if (nMinCellY < ORBG_GRID_ROWS) {
                    const int nMaxCellY = min(ORBG_GRID_ROWS - 1, (int)ceilf((v - K.min_y + r) * K.h_inv));
                    if (nMaxCellY >= 0 && nMaxCellX >= nMinCellX && nMaxCellY >= nMinCellY) {
                      sv.cells = nMinCellX | (nMaxCellX << 8) | (nMinCellY << 16) | (nMaxCellY << 24);
                      survives = true;
                    }
                  }
                }
              }
            }
          }
        }
      }
    }
    if (!survives) {
      const size_t o = (size_t)k * A.P + i;
      orbm_fuse_record r;
      r.status = status; r.best_idx = -1; r.best_dist = kInitDist; r.level = sv.level; r.n_cand = 0;
      A.rec[o] = r;
      uint4* c = reinterpret_cast<uint4*>(A.cand + o * kCap);
      c[0] = make_uint4(~0u, ~0u, ~0u, ~0u); c[1] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
  }
  // ---- the workgroup's survivor list, by ballot rank
  const unsigned long long bal = __ballot(survives);
  if (lane == 0) s_wcnt[wave] = __popcll(bal);
  __syncthreads();
  int woff = 0, nsurv = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; w++) { if (w < wave) woff += s_wcnt[w]; nsurv += s_wcnt[w]; }
  if (survives) s_surv[woff + __popcll(bal & ((1ull << lane) - 1ull))] = sv;
  __syncthreads();

  // ---- windows: 16 lanes per survivor
  const int sub = threadIdx.x & (kLanes - 1), grp = threadIdx.x / kLanes;
  for (int si = grp; si < nsurv; si += kGroups) {
    const Survivor s = s_surv[si];
    const int pi = blockIdx.x * kThreads + s.local;
    const size_t o = (size_t)k * A.P + pi;
    const int minX = s.cells & 255, maxX = (s.cells >> 8) & 255, minY = (s.cells >> 16) & 255, maxY = (s.cells >> 24) & 255;
    const int ncy = maxY - minY + 1, ncell = (maxX - minX + 1) * ncy;
    const uint4 a0 = *reinterpret_cast<const uint4*>(A.desc + (size_t)pi * 32);
    const uint4 a1 = *reinterpret_cast<const uint4*>(A.desc + (size_t)pi * 32 + 16);
    unsigned long long best = ~0ull;
    int n_win = 0, n_cand = 0;                     // group totals so far (the same in every lane of the group)
    for (int c0 = 0; c0 < ncell; c0 += kLanes) {
      const int c = c0 + sub;
      int b = 0, e = 0;
      if (c < ncell) {
        const int cell = (minX + c / ncy) * ORBG_GRID_ROWS + (minY + c % ncy);
        b = K.cell_start[cell]; e = K.cell_start[cell + 1];
      }
      int w_mine = 0, c_mine = 0;
      for (int j = b; j < e; j++) {
        bool in_w, is_c;
        classify<kSim3>(K, s, K.cell_items[j], &in_w, &is_c);
        w_mine += in_w; c_mine += is_c;
      }
      const int c_incl = group_incl_scan(c_mine, sub), w_incl = group_incl_scan(w_mine, sub);
      int rank = n_cand + c_incl - c_mine;
      for (int j = b; j < e && c_mine > 0; j++) {
        const int idx = K.cell_items[j];
        bool in_w, is_c;
        classify<kSim3>(K, s, idx, &in_w, &is_c);
        if (!is_c) continue;
        const uint4 b0 = *reinterpret_cast<const uint4*>(K.desc + (size_t)idx * 32);
        const uint4 b1 = *reinterpret_cast<const uint4*>(K.desc + (size_t)idx * 32 + 16);
        const unsigned long long key = ((unsigned long long)popc256(a0, a1, b0, b1) << 40) | ((unsigned long long)rank << 16) | (unsigned)idx;
        best = key < best ? key : best;
        if (rank < kCap) A.cand[o * kCap + rank] = (uint16_t)idx;
        rank++;
      }
      n_cand += __shfl(c_incl, kLanes - 1, kLanes);
      n_win += __shfl(w_incl, kLanes - 1, kLanes);
    }
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
      const unsigned long long other = __shfl_xor(best, m, kLanes);
      best = other < best ? other : best;
    }
    if (sub >= n_cand) A.cand[o * kCap + sub] = 0xFFFF;
    if (sub == 0) {
      orbm_fuse_record r;
      r.level = s.level; r.n_cand = n_cand;
      if (n_cand > 0) { r.status = ORBM_FUSE_CANDIDATES; r.best_idx = (int)(best & 0xFFFFu); r.best_dist = (int)(best >> 40); }
      else { r.status = n_win > 0 ? ORBM_FUSE_NO_CANDIDATE : ORBM_FUSE_EMPTY_WINDOW; r.best_idx = -1; r.best_dist = kInitDist; }
      A.rec[o] = r;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host

struct FuseBufs {
  orbg::StageBlock stage;
  orbg::DevBuf<orbm_fuse_record> d_rec;
  orbg::DevBuf<uint16_t> d_cand;
  orbg::PinnedBuf<orbm_fuse_record> h_rec;
  orbg::PinnedBuf<uint16_t> h_cand;
  std::vector<FuseKfDev> kf;
  std::vector<hipStream_t> streams;
  hipEvent_t ev = nullptr;
  void release_buffers() {
    stage.release(); d_rec.release(); d_cand.release(); h_rec.release(); h_cand.release();
    if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
  }
};

// the keyframe's pose as the kernel reads it.  Sim3 form: S/ORBmatcher.cc:1616-1620 as orbm_search_by_projection_sim3 decomposes
// Scw (scw from row 0 in double, entries scaled by (float)(1 / scw), Ow = -Rcw^T tcw with double accumulation)
void fill_pose(const orbm_fuse_kf& k, bool sim3, FuseKfDev* d) {
  if (!sim3) {
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) d->R[3 * i + j] = k.Tcw[4 * i + j];
      d->t[i] = k.Tcw[4 * i + 3];
      d->Ow[i] = k.Ow[i];
    }
    return;
  }
  double s2 = 0;
  for (int j = 0; j < 3; j++) s2 += (double)k.Scw[j] * (double)k.Scw[j];
  const float scw = (float)std::sqrt(s2);
  const float alpha = (float)(1.0 / (double)scw);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) d->R[3 * i + j] = k.Scw[4 * i + j] * alpha + 0.0f;
    d->t[i] = k.Scw[4 * i + 3] * alpha + 0.0f;
  }
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int j = 0; j < 3; j++) s += (double)d->R[3 * j + i] * (double)d->t[j];
    d->Ow[i] = (float)(-s);
  }
}

thread_local orbg::WorkArea<FuseBufs> t_area;

}  // namespace

extern "C" int orbm_fuse(const orbm_fuse_kf* kfs, int K, const orbm_worldpoints_view* pts, const uint8_t* skip, const orbm_fuse_params* params,
                         orbm_fuse_record* records, uint16_t* cand) {
  if (!params || params->struct_size != sizeof(orbm_fuse_params) || !pts || K < 0 || pts->m < 0 || (K > 0 && !kfs)) return ORBG_BAD_ARG;
  if (K > ORBG_FUSE_MAX_KEYFRAMES) return ORBG_CAP_EXCEEDED;
  const int P = pts->m;
  if (P > 0 && (!pts->pos || !pts->normal || !pts->min_dist || !pts->max_dist || !pts->desc)) return ORBG_BAD_ARG;
  if (K > 0 && P > 0 && (!records || !cand)) return ORBG_BAD_ARG;
  const bool sim3 = params->sim3_form != 0;
  orbg::WorkArea<FuseBufs>& W = t_area;
  W.kf.resize(K);
  W.streams.clear();
  int device = -1;
  for (int k = 0; k < K; k++) {
    const orbm_fuse_kf& q = kfs[k];
    if (q.struct_size != sizeof(orbm_fuse_kf) || !q.frame) return ORBG_BAD_ARG;
    if (q.n_levels < 1 || q.n_levels > ORBG_MAX_LEVELS || !q.scale_factors || !q.inv_level_sigma2) return ORBG_BAD_ARG;
    FuseKfDev& d = W.kf[k];
    const float* d_depth; const orbx_keypoint* h_kps; int n, dev; hipStream_t st;      // (depth and the host mirror are not read here)
    int rc = orbm_internal_kf_features(q.frame, &d.kps, &d.desc, &d.uright, &d_depth, &h_kps, &n, &dev, &st);
    if (rc) return rc;
    if (n >= ORBG_MAX_FRAME_FEATURES) return ORBG_CAP_EXCEEDED;      // indices travel as uint16 (cand, the reduction key), 0xFFFF = unused
    if (device < 0) device = dev;
    else if (dev != device) return ORBG_BAD_ARG;
    FrameParams fp;
    if ((rc = orbm_internal_kf_grid(q.frame, &d.cell_start, &d.cell_items, &fp))) return rc;
    fill_pose(q, sim3, &d);
    d.fx = q.fx; d.fy = q.fy; d.cx = q.cx; d.cy = q.cy; d.bf = q.mbf;
    d.min_x = fp.min_x; d.max_x = fp.max_x; d.min_y = fp.min_y; d.max_y = fp.max_y; d.w_inv = fp.w_inv; d.h_inv = fp.h_inv;
    d.log_sf = q.log_scale_factor; d.n_levels = q.n_levels;
    for (int l = 0; l < ORBG_MAX_LEVELS; l++) {
      d.sf[l] = l < q.n_levels ? q.scale_factors[l] : 0.f;
      d.inv_sigma2[l] = l < q.n_levels ? q.inv_level_sigma2[l] : 0.f;
    }
    if (std::find(W.streams.begin(), W.streams.end(), st) == W.streams.end()) W.streams.push_back(st);
  }
  if (K == 0 || P == 0) return ORBG_OK;
  int rc;
  if ((rc = W.open(device, "misc"))) return rc;
  if (!W.ev) ORBG_HIP(hipEventCreateWithFlags(&W.ev, hipEventDisableTiming));
  const size_t nrec = (size_t)K * (size_t)P;
  // one pinned block, one H2D copy: FuseKfDev[K], the points, the skip bytes
  const bool pskip = pts->bad || pts->skip;
  orbg::StageBlock& S = W.stage;
  if ((rc = S.begin(orbg::StageLayout::bound(8, (size_t)K * sizeof(FuseKfDev) + (size_t)P * 65 + nrec))) || (rc = W.d_rec.reserve(nrec)) ||
      (rc = W.d_cand.reserve(nrec * kCap)) || (rc = W.h_rec.reserve(nrec)) || (rc = W.h_cand.reserve(nrec * kCap)))
    return rc;
  FuseArgs A;
  A.kf = S.add(W.kf.data(), K, true);
  A.pos = S.add(pts->pos, 3 * (size_t)P, true); A.normal = S.add(pts->normal, 3 * (size_t)P, true);
  A.min_dist = S.add(pts->min_dist, P, true); A.max_dist = S.add(pts->max_dist, P, true);
  A.desc = S.add(pts->desc, 32 * (size_t)P, true);
  A.pskip = nullptr;
  if (pskip) {
    const auto s_ps = S.room<uint8_t>(P, true);
    for (int i = 0; i < P; i++) S.host(s_ps)[i] = (uint8_t)((pts->bad && pts->bad[i]) || (pts->skip && pts->skip[i]));
    A.pskip = S.device(s_ps);
  }
  A.skip = skip ? S.add(skip, nrec, true) : nullptr;
  A.rec = W.d_rec.p; A.cand = W.d_cand.p;
  A.P = P; A.th = params->th;
  // the calling thread's stream; what is pending on the keyframes' streams (an upload, a constructor) is ordered in front
  hipStream_t st = W.stream;
  orbg::StreamDrain drain{st};
  for (hipStream_t fs : W.streams) {
    if (fs == st) continue;
    ORBG_HIP(hipEventRecord(W.ev, fs));
    ORBG_HIP(hipStreamWaitEvent(st, W.ev, 0));
  }
  if ((rc = S.commit(st))) return rc;
  const dim3 grid((P + kThreads - 1) / kThreads, K);
  if (sim3) hipLaunchKernelGGL(fuse_kernel<true>, grid, dim3(kThreads), 0, st, A);
  else hipLaunchKernelGGL(fuse_kernel<false>, grid, dim3(kThreads), 0, st, A);
  ORBG_HIP(hipGetLastError());
  ORBG_HIP(hipMemcpyAsync(W.h_rec.h, W.d_rec.p, nrec * sizeof(orbm_fuse_record), hipMemcpyDeviceToHost, st));
  ORBG_HIP(hipMemcpyAsync(W.h_cand.h, W.d_cand.p, nrec * kCap * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  ORBG_HIP(hipStreamSynchronize(st));
  memcpy(records, W.h_rec.h, nrec * sizeof(orbm_fuse_record));           // (the caller's arrays are pageable: a direct copy would pin them per call)
  memcpy(cand, W.h_cand.h, nrec * kCap * sizeof(uint16_t));
  return ORBG_OK;
}
