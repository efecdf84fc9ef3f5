// ORBmatcher::SearchForInitialization (S/ORBmatcher.cc:702-817): the matcher of Tracking::MonocularInitialization
// (S/Tracking.cc:2217).  For every octave-0 feature of F1 the device gathers the candidate list Frame::GetFeaturesInArea
// (S/Frame.cc:628-697) returns around vbPrevMatched[i1], in the reference's order and with the Hamming distance of every entry;
// the serial rules (the vMatchedDistance skip, best / second best, the ratio test, evictions, the rotation vote, the update of
// vbPrevMatched) run on the host over those lists (init_replay.hpp).  No tickets, no spin-waits, no ordering between workgroups.
//
// Level-0 view.  Both the queries and the candidates are octave-0 features only (:719, :722 with minLevel = maxLevel = 0), one in
// five of a frame.  l0_view_kernel filters the frame's grid (CSR, cell = ix * 48 + iy, ascending feature index inside a cell) down to
// those features: a CSR over the same 3072 cells, and x, y, angle, original index and descriptor gathered in CSR order.  Filtering
// keeps the relative order, and cells of one ix are consecutive, so the reference's candidate order for a window is the
// concatenation, over ix = nMinCellX .. nMaxCellX, of ONE contiguous range each (iy = nMinCellY .. nMaxCellY): at most 64 ranges.
// The view is built once per frame content and kept on the orbm_frame (matcher.hip counts the content changes); its host mirror
// (x, y, angle, original index) arrives with the first call's results.
//
// Search.  One wavefront per feature of F1, four per workgroup.  Lane j owns range j: its length comes from two reads of the view's
// CSR, a wavefront scan gives the range's offset in the list and the list's upper bound (every level-0 feature of the touched cells).
// One atomic add on a cursor reserves that many entries of the candidate buffer in HBM -- the only atomic, and it decides where a
// list lies, never what it holds.  Then the lanes walk the concatenation 64 positions at a time: a position finds its range by a
// six-step search of the offsets in LDS, loads x / y (coalesced inside a range), applies the strict window test (:690), and a
// survivor loads its 32-byte descriptor and takes the popcount of the XOR.  A ballot and a prefix count compact the survivors
// behind the list's running end, so the order is the reference's.  A record per feature holds base, count and the angle.
//
// Capacity.  A query whose reservation does not fit writes nothing, but the cursor still counts: the host sees the total, grows the
// buffer to it and runs the search again (n_regrown).  Nothing is ever truncated; only ORBM_INIT_SEARCH_MAX_LIST answers
// ORBG_CAP_EXCEEDED.
//
// Arithmetic: the cell bounds are float32, left to right, as S/Frame.cc:639-657 writes them ((x - mnMinX - r) * mfGridElementWidthInv,
// floor / ceil, then the clamps and the four early returns); everything else is integer.  Two runs give the same lists.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "grid_build.hpp"
#include "init_replay.hpp"

using orbg::FrameParams;
using orbg::kCells;

// matcher.hip
int orbm_internal_kf_features(orbm_frame* f, const orbx_keypoint** d_kps, const uint8_t** d_desc, const float** d_uright,
                              const float** d_depth, const orbx_keypoint** h_kps, int* n, int* device, hipStream_t* stream);
int orbm_internal_kf_grid(orbm_frame* f, const int** d_cell_start, const int** d_cell_items, FrameParams* fp);
int orbm_internal_order_after(orbm_frame* f, hipStream_t st);
int orbm_internal_side_cache(orbm_frame* f, unsigned* content_gen, void*** slot, void (***free_fn)(void*));

namespace {

constexpr int kViewThreads = 1024;
constexpr int kSearchThreads = 256;
constexpr int kWaves = kSearchThreads / 64;
constexpr size_t kDefaultListCap = (size_t)1 << 20;

struct L0Item { float x, y, angle; int idx; };      // one octave-0 feature of the view, CSR order
struct InitRec { int base, count; float angle; };   // per feature of F1; count < 0: no query

// ------------------------------------------------------------------------------------------------ level-0 view

__global__ __launch_bounds__(kViewThreads) void l0_view_kernel(const orbx_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                              const int* __restrict__ cell_start, const int* __restrict__ cell_items,
                                                              int n, int* __restrict__ l0_start, L0Item* __restrict__ item,
                                                              uint4* __restrict__ l0_desc) {
  constexpr int CPT = kCells / kViewThreads;
  static_assert(kCells % kViewThreads == 0, "a thread owns CPT consecutive cells");
  __shared__ int wsum[kViewThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = tid * CPT;
  int cnt[CPT];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    const int s = cell_start[c0 + k], e = min(cell_start[c0 + k + 1], n);
    int c = 0;
    for (int j = s; j < e; j++) {
      const int it = cell_items[j];
      if ((unsigned)it < (unsigned)n && kps[it].octave == 0) c++;
    }
    cnt[k] = c;
    mine += c;
  }
  const int inc = orbg::wave_incl_scan_add(mine);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int run = inc - mine;
  for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    l0_start[c0 + k] = run;
    if (cnt[k] == 0) continue;
    const int s = cell_start[c0 + k], e = min(cell_start[c0 + k + 1], n);
    for (int j = s; j < e; j++) {
      const int it = cell_items[j];
      if ((unsigned)it >= (unsigned)n) continue;
      const orbx_keypoint kp = kps[it];
      if (kp.octave != 0) continue;
      if (run < n) {
        L0Item o; o.x = kp.x; o.y = kp.y; o.angle = kp.angle; o.idx = it;
        item[run] = o;
        const uint4* d = reinterpret_cast<const uint4*>(desc + (size_t)it * 32);
        l0_desc[2 * run] = d[0];
        l0_desc[2 * run + 1] = d[1];
      }
      run++;
    }
  }
  if (tid == kViewThreads - 1) l0_start[kCells] = min(run, n);
}

// ------------------------------------------------------------------------------------------------ search

struct InitSearchArgs {
  const orbx_keypoint* kps1; const uint8_t* desc1; const float* prev;   // F1: mvKeysUn, mDescriptors; vbPrevMatched (n1 x {x, y})
  int n1;
  const int* l0_start; const L0Item* item; const uint4* l0_desc;       // the level-0 view of F2
  float min_x, min_y, w_inv, h_inv, r;
  InitRec* rec;                  // n1
  uint32_t* entries;             // cap
  unsigned cap;
  unsigned* cursor;              // entries reserved so far (upper bounds); beyond cap: the total a second run needs
};

__device__ __forceinline__ int popc256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// float -> int of a cell coordinate, clamped first: beyond +-1e9 the cell is outside the grid on that side whatever its value
__device__ __forceinline__ int cell_of(float v) { return (int)fminf(fmaxf(v, -1.0e9f), 1.0e9f); }

__global__ __launch_bounds__(kSearchThreads) void init_search_kernel(InitSearchArgs A) {
  __shared__ int s_off[kWaves][64];      // offset of range j in the concatenation (exclusive prefix of the lengths)
  __shared__ int s_src[kWaves][64];      // first view position of range j
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * kWaves + wave;
  // everything up to the barrier is wavefront-uniform except the lane's own range
  bool query = false, window = false;
  float qx = 0.f, qy = 0.f, angle = 0.f;
  int minCX = 0, minCY = 0, maxCY = 0, ncol = 0;
  if (q < A.n1) {
    const orbx_keypoint kp = A.kps1[q];
    angle = kp.angle;
    query = kp.octave == 0;                                                      // :718-720
    if (query) {
      qx = A.prev[2 * q]; qy = A.prev[2 * q + 1];
      // S/Frame.cc:639-661.  cell_of keeps the conversion inside int: a wild query point (or a NaN) ends at an early return
      minCX = max(0, cell_of(floorf((qx - A.min_x - A.r) * A.w_inv)));
      const int maxCX = min(ORBG_GRID_COLS - 1, cell_of(ceilf((qx - A.min_x + A.r) * A.w_inv)));
      minCY = max(0, cell_of(floorf((qy - A.min_y - A.r) * A.h_inv)));
      maxCY = min(ORBG_GRID_ROWS - 1, cell_of(ceilf((qy - A.min_y + A.r) * A.h_inv)));
      window = !(minCX >= ORBG_GRID_COLS || maxCX < 0 || minCY >= ORBG_GRID_ROWS || maxCY < 0) && maxCX >= minCX && maxCY >= minCY;
      ncol = window ? maxCX - minCX + 1 : 0;
    }
  }
  int src = 0, len = 0;
  if (lane < ncol) {
    const int c = (minCX + lane) * ORBG_GRID_ROWS;
    src = A.l0_start[c + minCY];
    len = A.l0_start[c + maxCY + 1] - src;
  }
  const int inc = orbg::wave_incl_scan_add(len);
  const int ub = __builtin_amdgcn_readlane(inc, 63);
  s_off[wave][lane] = lane < ncol ? inc - len : INT_MAX;      // (lanes past the last range never win the search)
  s_src[wave][lane] = src;
  __syncthreads();
  if (q >= A.n1) return;
  if (!query || ub == 0) {
    if (lane == 0) { InitRec r; r.base = 0; r.count = query ? 0 : -1; r.angle = angle; A.rec[q] = r; }
    return;
  }
  unsigned base = 0;
  if (lane == 0) base = atomicAdd(A.cursor, (unsigned)ub);
  base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
  if (base > A.cap || (unsigned)ub > A.cap - base) {            // does not fit: counted, not written; the host runs the search again
    if (lane == 0) { InitRec r; r.base = 0; r.count = 0; r.angle = angle; A.rec[q] = r; }
    return;
  }
  const uint4* qd = reinterpret_cast<const uint4*>(A.desc1 + (size_t)q * 32);
  const uint4 q0 = qd[0], q1 = qd[1];
  const int* off = s_off[wave];
  int count = 0;
  for (int cb = 0; cb < ub; cb += 64) {
    const int p = cb + lane;
    bool pass = false;
    int pos = 0, dist = 0;
    if (p < ub) {
      int j = 0;
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1)
        if (off[j + step] <= p) j += step;
      pos = s_src[wave][j] + (p - off[j]);
      const L0Item it = A.item[pos];
      pass = fabsf(it.x - qx) < A.r && fabsf(it.y - qy) < A.r;                    // S/Frame.cc:687-690
      if (pass) dist = popc256(q0, q1, A.l0_desc[2 * pos], A.l0_desc[2 * pos + 1]);
    }
    const unsigned long long m = __ballot(pass);
    if (pass) A.entries[base + count + __popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)pos | ((uint32_t)dist << 16);
    count += __popcll(m);
  }
  if (lane == 0) { InitRec r; r.base = (int)base; r.count = count; r.angle = angle; A.rec[q] = r; }
}

// ------------------------------------------------------------------------------------------------ host

// what a frame keeps for this search (matcher.hip owns the slot and calls view_free when the frame goes)
struct L0View {
  unsigned gen = 0;
  bool counted = false, on_device = false, on_host = false;
  int n = 0;                                 // features
  int n_oct0 = 0;                            // octave-0 features, counted on the host: what the frame asks as F1 (a query needs no cell)
  int n_view = 0;                            // those of them inside the grid, counted by the kernel: what the view holds (with on_host)
  orbg::DevBuf<int> d_start;
  orbg::DevBuf<L0Item> d_item;
  orbg::DevBuf<uint4> d_desc;
  orbg::PinnedBuf<L0Item> h_item;
  orbg::PinnedBuf<int> h_n0;
  std::vector<float> angle, pt;              // the mirror split for the replay: n_view, n_view x {x, y}
  std::vector<int> idx;                      // view position -> feature index
};

void view_free(void* p) {
  L0View* v = static_cast<L0View*>(p);
  v->d_start.release(); v->d_item.release(); v->d_desc.release(); v->h_item.release(); v->h_n0.release();
  delete v;
}

// the frame's view for its current content: a new content forgets what was built; n_oct0 is counted on the host mirror of the keypoints
int view_of(orbm_frame* f, const orbx_keypoint* hk, int n, L0View** out) {
  unsigned gen; void** slot; void (**free_fn)(void*);
  int rc = orbm_internal_side_cache(f, &gen, &slot, &free_fn);
  if (rc) return rc;
  if (!*slot) { *slot = new L0View(); *free_fn = view_free; }
  L0View* v = static_cast<L0View*>(*slot);
  if (!v->counted || v->gen != gen || v->n != n) {
    v->gen = gen; v->n = n; v->on_device = v->on_host = false;
    int n0 = 0;
    if (n > 0 && !hk) return ORBG_BAD_ARG;
    for (int i = 0; i < n; i++) n0 += hk[i].octave == 0;
    v->n_oct0 = n0; v->n_view = 0; v->counted = true;
  }
  *out = v;
  return ORBG_OK;
}

struct InitBufs {
  orbg::PinnedBuf<float> h_prev;
  orbg::DevBuf<float> d_prev;
  orbg::DevBuf<InitRec> d_rec;
  orbg::PinnedBuf<InitRec> h_rec;
  orbg::DevBuf<uint32_t> d_entries;
  orbg::PinnedBuf<uint32_t> h_entries;
  orbg::DevBuf<unsigned> d_cursor;
  orbg::PinnedBuf<unsigned> h_cursor;
  std::vector<int32_t> base, count, m12;
  std::vector<float> angle1;
  orbg::InitReplayScratch scratch;
  void release_buffers() {
    h_prev.release(); d_prev.release(); d_rec.release(); h_rec.release(); d_entries.release(); h_entries.release(); d_cursor.release();
    h_cursor.release();
  }
};

thread_local orbg::WorkArea<InitBufs> t_area;

}  // namespace

extern "C" int orbm_search_for_initialization(orbm_frame* f1, orbm_frame* f2, float* prev_matched, int n_prev,
                                              const orbm_init_search_params* params, int32_t* matches12, int* n_matches,
                                              orbm_init_search_debug* debug) {
  if (!f1 || !f2 || !params || !n_matches || n_prev < 0) return ORBG_BAD_ARG;
  if (params->struct_size < sizeof(orbm_init_search_params) || params->window_size <= 0 || params->list_capacity < 0) return ORBG_BAD_ARG;
  if (n_prev > 0 && (!prev_matched || !matches12)) return ORBG_BAD_ARG;
  if (debug && (!debug->list_start || debug->entries_cap < 0 || (debug->entries_cap > 0 && !debug->entries))) return ORBG_BAD_ARG;
  const orbx_keypoint *dk1, *dk2, *hk1, *hk2; const uint8_t *dd1, *dd2; const float *du, *dz; int n1, n2, dev1, dev2; hipStream_t s1, s2;
  int rc;
  if ((rc = orbm_internal_kf_features(f1, &dk1, &dd1, &du, &dz, &hk1, &n1, &dev1, &s1))) return rc;
  if ((rc = orbm_internal_kf_features(f2, &dk2, &dd2, &du, &dz, &hk2, &n2, &dev2, &s2))) return rc;
  if (dev1 != dev2 || n_prev != n1) return ORBG_BAD_ARG;
  if ((rc = orbg::select_device(dev1))) return rc;
  L0View *v1, *v2;
  if ((rc = view_of(f1, hk1, n1, &v1)) || (rc = view_of(f2, hk2, n2, &v2))) return rc;
  *n_matches = 0;
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  if (debug) {
    for (int i = 0; i <= n1; i++) debug->list_start[i] = 0;
    debug->n_queries = v1->n_oct0; debug->n_candidates = debug->n_evictions = debug->n_rot_rejected = debug->n_regrown = 0;
  }
  if (v1->n_oct0 == 0 || v2->n_oct0 == 0) return ORBG_OK;                 // (covers n1 == 0 and n2 == 0): no launch
  const int* d_cell_start; const int* d_cell_items; FrameParams fp;
  if ((rc = orbm_internal_kf_grid(f2, &d_cell_start, &d_cell_items, &fp))) return rc;
  orbg::WorkArea<InitBufs>& W = t_area;
  if ((rc = W.open(dev1, "misc"))) return rc;
  size_t cap = params->list_capacity > 0 ? (size_t)params->list_capacity : std::max(kDefaultListCap, W.d_entries.cap);
  if (cap > ORBM_INIT_SEARCH_MAX_LIST) cap = ORBM_INIT_SEARCH_MAX_LIST;
  if ((rc = W.h_prev.reserve((size_t)n1 * 2)) || (rc = W.d_prev.reserve((size_t)n1 * 2)) || (rc = W.d_rec.reserve(n1)) ||
      (rc = W.h_rec.reserve(n1)) || (rc = W.d_entries.reserve(cap)) || (rc = W.d_cursor.reserve(1)) || (rc = W.h_cursor.reserve(1)))
    return rc;
  if (!v2->on_device &&
      ((rc = v2->d_start.reserve(kCells + 1)) || (rc = v2->d_item.reserve(n2)) || (rc = v2->d_desc.reserve((size_t)n2 * 2)) ||
       (rc = v2->h_item.reserve(n2)) || (rc = v2->h_n0.reserve(1))))
    return rc;
  // the calling thread's stream, behind what is pending on the frames' streams (an upload, a constructor, the grid build)
  hipStream_t st = W.stream;
  orbg::StreamDrain drain{st};
  if ((rc = orbm_internal_order_after(f1, st)) || (rc = orbm_internal_order_after(f2, st))) return rc;
  memcpy(W.h_prev.h, prev_matched, (size_t)n1 * 2 * sizeof(float));
  ORBG_HIP(hipMemcpyAsync(W.d_prev.p, W.h_prev.h, (size_t)n1 * 2 * sizeof(float), hipMemcpyHostToDevice, st));
  if (!v2->on_device) {
    hipLaunchKernelGGL(l0_view_kernel, dim3(1), dim3(kViewThreads), 0, st, dk2, dd2, d_cell_start, d_cell_items, n2, v2->d_start.p,
                       v2->d_item.p, v2->d_desc.p);
    ORBG_HIP(hipGetLastError());
    ORBG_HIP(hipMemcpyAsync(v2->h_item.h, v2->d_item.p, (size_t)v2->n_oct0 * sizeof(L0Item), hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipMemcpyAsync(v2->h_n0.h, v2->d_start.p + kCells, sizeof(int), hipMemcpyDeviceToHost, st));
    v2->on_device = true;
  }
  InitSearchArgs A;
  A.kps1 = dk1; A.desc1 = dd1; A.prev = W.d_prev.p; A.n1 = n1;
  A.l0_start = v2->d_start.p; A.item = v2->d_item.p; A.l0_desc = v2->d_desc.p;
  A.min_x = fp.min_x; A.min_y = fp.min_y; A.w_inv = fp.w_inv; A.h_inv = fp.h_inv; A.r = (float)params->window_size;
  A.rec = W.d_rec.p; A.cursor = W.d_cursor.p;
  int regrown = 0;
  unsigned total = 0;
  for (;;) {
    A.entries = W.d_entries.p; A.cap = (unsigned)cap;
    ORBG_HIP(hipMemsetAsync(W.d_cursor.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(init_search_kernel, dim3((n1 + kWaves - 1) / kWaves), dim3(kSearchThreads), 0, st, A);
    ORBG_HIP(hipGetLastError());
    ORBG_HIP(hipMemcpyAsync(W.h_rec.h, W.d_rec.p, (size_t)n1 * sizeof(InitRec), hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipMemcpyAsync(W.h_cursor.h, W.d_cursor.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipStreamSynchronize(st));                            // first wait: the records and the total
    total = W.h_cursor.h[0];
    if ((size_t)total <= cap) break;
    if ((size_t)total > ORBM_INIT_SEARCH_MAX_LIST || regrown) return regrown ? ORBG_INTERNAL : ORBG_CAP_EXCEEDED;
    cap = total;                                                   // the lists did not fit: grow to what the kernel counted, search again
    if ((rc = W.d_entries.reserve(cap))) return rc;
    regrown++;
  }
  if (!v2->on_host) {                                              // the mirror came with the first wait
    const int n0 = v2->h_n0.h[0];                                  // (a feature outside the image bounds is in no cell, S/Frame.cc:699-709)
    if (n0 < 0 || n0 > v2->n_oct0) return ORBG_INTERNAL;
    v2->n_view = n0;
    v2->angle.resize(n0); v2->pt.resize((size_t)n0 * 2); v2->idx.resize(n0);
    for (int i = 0; i < n0; i++) {
      const L0Item& it = v2->h_item.h[i];
      if ((unsigned)it.idx >= (unsigned)n2) return ORBG_INTERNAL;
      v2->angle[i] = it.angle; v2->pt[2 * i] = it.x; v2->pt[2 * i + 1] = it.y; v2->idx[i] = it.idx;
    }
    v2->on_host = true;
  }
  if (total > 0) {
    if ((rc = W.h_entries.reserve(total))) return rc;
    ORBG_HIP(hipMemcpyAsync(W.h_entries.h, W.d_entries.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ORBG_HIP(hipStreamSynchronize(st));                            // second wait: the lists
  }
  W.base.resize(n1); W.count.resize(n1); W.angle1.resize(n1); W.m12.resize(n1);
  for (int i = 0; i < n1; i++) {
    const InitRec& r = W.h_rec.h[i];
    if (r.count > 0 && ((unsigned)r.base > total || (unsigned)r.count > total - (unsigned)r.base)) return ORBG_INTERNAL;
    W.base[i] = r.base; W.count[i] = r.count; W.angle1[i] = r.angle;
  }
  orbg::InitReplayCounters ctr;
  const int nm = orbg::init_search_replay(n1, v2->n_view, W.base.data(), W.count.data(), W.h_entries.h, W.angle1.data(), v2->angle.data(),
                                          v2->pt.data(), params->nn_ratio, params->check_orientation != 0, prev_matched, W.m12.data(),
                                          W.scratch, &ctr);
  for (int i = 0; i < n1; i++) matches12[i] = W.m12[i] >= 0 ? v2->idx[W.m12[i]] : -1;
  *n_matches = nm;
  if (debug) {
    debug->n_queries = ctr.n_queries; debug->n_candidates = ctr.n_candidates; debug->n_evictions = ctr.n_evictions;
    debug->n_rot_rejected = ctr.n_rot_rejected; debug->n_regrown = regrown;
    int run = 0;
    for (int i = 0; i < n1; i++) { debug->list_start[i] = run; run += std::max(W.count[i], 0); }
    debug->list_start[n1] = run;
    if (run > debug->entries_cap) return ORBG_CAP_EXCEEDED;        // (every other output is complete: call again with n_candidates entries)
    for (int i = 0; i < n1; i++) {
      const uint32_t* e = W.h_entries.h + W.base[i];
      uint32_t* o = debug->entries + debug->list_start[i];
      for (int k = 0; k < W.count[i]; k++) o[k] = (uint32_t)v2->idx[e[k] & 0xFFFFu] | (e[k] & 0xFFFF0000u);
    }
  }
  return ORBG_OK;
}
