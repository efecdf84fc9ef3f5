// Shared host-side helpers for liborbgpu (HIP runtime only; no torch, no third-party deps).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/orbgpu.h"
#include "stage_layout.hpp"

#define ORBG_HIP(expr)                                                                          \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      if (getenv("ORBG_VERBOSE"))                                                               \
        fprintf(stderr, "[orbgpu] %s:%d %s -> %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return (_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? ORBG_NO_DEVICE : ORBG_HIP_ERROR; \
    }                                                                                           \
  } while (0)

namespace orbg {

constexpr int kEdge = 19;        // EDGE_THRESHOLD  S/ORBextractor.cc:72
constexpr int kHalfPatch = 15;   // HALF_PATCH_SIZE S/ORBextractor.cc:71
constexpr int kPatch = 31;       // PATCH_SIZE      S/ORBextractor.cc:70

// ORBG_POISON=1 fills every new buffer with 0xA5 so that a kernel consuming memory nobody wrote shows up in the parity
// tests (fresh HIP allocations are often zero, recycled ones are not).  Test aid; allocations are outside the timed path.
inline bool poison_allocations() { static const bool on = getenv("ORBG_POISON") != nullptr; return on; }

// Wait policy per host-thread ROLE (include/orbgpu.h, "Host threads"): a wait either SPINS on a completion word in pinned memory or
// goes through the runtime's blocking waits / a condition variable.  Roles: the caller's threads (Tracking), the local-BA worker of a
// handle, the process's image-ingest thread.  ORBG_NO_POLL in the environment gives the start-up policy ("1" / "all": every role
// blocks; a comma list of caller / lba / ingest: those roles block); orbg_set_wait_policy() changes it at run time.  Implemented in
// misc.cpp (one state for all translation units); poll_allowed() is what every wait site asks -- an atomic load + a thread-local.
enum { kRoleCaller = 0, kRoleLbaWorker = 1, kRoleIngest = 2, kRoleCount = 3 };
bool poll_allowed();                 // may the CALLING thread spin?
void set_thread_role(int role);      // called once by the library's own threads when they start

// Growable device buffer (never shrinks); all allocations happen outside the timed/launch path once sizes settle.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;                  // an owner: overwriting one would lose its allocation
  DevBuf& operator=(const DevBuf&) = delete;
  int reserve(size_t n) {
    if (n <= cap) return ORBG_OK;
    if (p) { ORBG_HIP(hipFree(p)); p = nullptr; cap = 0; }
    size_t want = n + n / 4 + 64;
    ORBG_HIP(hipMalloc((void**)&p, want * sizeof(T)));
    // (the fill runs on the null stream and hipMemset may return before it has finished; the library's streams are non-blocking
    // since round 4 and do not join it: without the synchronisation the fill raced with the first kernels that write the buffer)
    if (poison_allocations()) { ORBG_HIP(hipMemset(p, 0xA5, want * sizeof(T))); ORBG_HIP(hipDeviceSynchronize()); }
    cap = want;
    return ORBG_OK;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
};

// Pinned host buffer that the device can address directly (zero-copy hand-off of small, latency-bound records).
template <typename T>
struct PinnedBuf {
  T* h = nullptr;
  T* d = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  int reserve(size_t n) {
    if (n <= cap) return ORBG_OK;
    if (h) { ORBG_HIP(hipHostFree(h)); h = nullptr; d = nullptr; cap = 0; }
    size_t want = n + n / 4 + 64;
    ORBG_HIP(hipHostMalloc((void**)&h, want * sizeof(T), hipHostMallocMapped));
    ORBG_HIP(hipHostGetDevicePointer((void**)&d, h, 0));
    if (poison_allocations()) memset(h, 0xA5, want * sizeof(T));
    cap = want;
    return ORBG_OK;
  }
  void release() { if (h) { (void)hipHostFree(h); h = nullptr; d = nullptr; cap = 0; } }
};

// The staging block of an entry point: per-call arrays packed into ONE pinned block at the slots of a StageLayout, read by the kernel
// in place (mapped) or from the device block after ONE copy; results come back through slots of the same block.  The one place where
// a byte offset becomes a T*.
struct StageBlock {
  PinnedBuf<uint8_t> pin;
  DevBuf<uint8_t> dev;
  StageLayout lay;                       // single-pass form (begin .. commit)
  size_t dirty_lo = 0, dirty_hi = 0;     // part of the block that commit() copies to the device
  int reserve(size_t bytes) { int rc = pin.reserve(bytes); return rc ? rc : dev.reserve(bytes); }   // (growth as PinnedBuf / DevBuf)
  template <typename T> T* host(StageSlot<T> s) const { return reinterpret_cast<T*>(pin.h + s.off); }
  template <typename T> T* mapped(StageSlot<T> s) const { return reinterpret_cast<T*>(pin.d + s.off); }   // the device's address of host(s)
  template <typename T> T* device(StageSlot<T> s) const { return reinterpret_cast<T*>(dev.p + s.off); }
  template <typename T> void put(StageSlot<T> s, const T* src) { if (s.count) memcpy(host(s), src, s.bytes()); }
  template <typename T> void get(StageSlot<T> s, T* dst) const { if (s.count) memcpy(dst, host(s), s.bytes()); }
  // bytes [lo, hi) of the block, pinned -> device and back: one copy command each
  int upload(size_t lo, size_t hi, hipStream_t st) { ORBG_HIP(hipMemcpyAsync(dev.p + lo, pin.h + lo, hi - lo, hipMemcpyHostToDevice, st)); return ORBG_OK; }
  int download(size_t lo, size_t hi, hipStream_t st) { ORBG_HIP(hipMemcpyAsync(pin.h + lo, dev.p + lo, hi - lo, hipMemcpyDeviceToHost, st)); return ORBG_OK; }
  void release() { pin.release(); dev.release(); }
  // Single pass, for a site that lays out while it fills: `bound` >= the bytes the slots will take (StageLayout::bound).
  int begin(size_t bound) { lay = StageLayout(); dirty_lo = dirty_hi = 0; return reserve(bound); }
  // the next slot; dev_copy: it is part of what commit() uploads (inputs that many threads re-read), else it is read or written in place
  template <typename T> StageSlot<T> room(size_t count, bool dev_copy = false) {
    const StageSlot<T> s = lay.add<T>(count);
    if (dev_copy && count) { if (dirty_hi == dirty_lo) dirty_lo = s.off; dirty_hi = s.end(); }
    return s;
  }
  template <typename T> const T* add(const T* src, size_t count, bool dev_copy = false) {
    const StageSlot<T> s = room<T>(count, dev_copy);
    put(s, src);
    return dev_copy ? device(s) : mapped(s);
  }
  int commit(hipStream_t st) { return dirty_hi > dirty_lo ? upload(dirty_lo, dirty_hi, st) : ORBG_OK; }
};

// Completion signal without the runtime's wake-up path: a one-thread kernel at the tail of a stream writes a sequence number
// into mapped pinned memory (everything launched before it on that stream has completed and is visible by then), the host
// spins on that word.  Falls back to hipStreamSynchronize if the word does not arrive.
struct StreamSignal {
  PinnedBuf<unsigned> word;
  unsigned seq = 0;
  StreamSignal() = default;
  StreamSignal(const StreamSignal&) = delete;
  StreamSignal& operator=(const StreamSignal&) = delete;
  int init() { int rc = word.reserve(16); if (rc) return rc; word.h[0] = 0; return ORBG_OK; }
  void release() { word.release(); seq = 0; }   // (init() zeroes the next word: the count starts over with it)
  int post(hipStream_t st);      // enqueue the signal kernel (misc.cpp)
  // for kernels that post the signal themselves (DoneSig below): next sequence number + the word's device address
  int arm(unsigned* seq_out, volatile unsigned** flag_out) {
    if (!word.h) { int rc = init(); if (rc) return rc; }
    *seq_out = ++seq; *flag_out = (volatile unsigned*)word.d;
    return ORBG_OK;
  }
  int wait(hipStream_t st);      // spin until the posted signal arrives (misc.cpp)
  int sync(hipStream_t st) { int rc = post(st); return rc ? rc : wait(st); }
};

// The completion word of a solve that runs in ONE launch (pose_opt.hip, pose_inertial.hip, inertial_init.hip): an int inside the
// result record in mapped pinned memory, so that the record and its completion arrive with the same write-back.  The host side is one
// object per call site (static thread_local): arm() zeroes the word and issues the next sequence number, 31 bits and never 0, which
// the launch takes along; wait() spins on the word.  Kept apart from StreamSignal::wait on purpose: the two pace their spins differently
// (that one pauses in every spin, reads the clock every 0x4000 spins and gives up after 50 ms; this one does not pause, reads it every
// 0x10000 spins and gives up after 100 ms), both run on the tracking thread, and one loop for both would change the timing of one.
struct SolveWord {
  unsigned seq = 0;
  volatile const int* word = nullptr;
  unsigned arm(int* host_word) {
    seq = (seq + 1) & 0x7FFFFFFFu;
    if (seq == 0) seq = 1;
    *host_word = 0;
    word = host_word;
    return seq;
  }
  int wait(hipStream_t st) const;  // spin while poll_allowed(), then hipStreamSynchronize if the word has not arrived (misc.cpp)
};
// the kernel's last lines: every wavefront's results released to the system (no acquire half), then the word, by thread 0 alone
__device__ __forceinline__ void solve_word_complete(int* word, unsigned seq) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __syncthreads();
  if (threadIdx.x == 0) *reinterpret_cast<volatile int*>(word) = (int)seq;   // results are complete: the host spins on this word
}

// Streams of the library's handles.  HIP multiplexes the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (4 unless the
// environment says otherwise): the first four streams get a queue each, every further one joins the queue with the fewest users,
// ties broken by the queues' ADDRESSES -- i.e. differently from run to run.  Streams that share a hardware queue are serialised: with
// one stream per handle (two extractors, two frames, the local map, the local BA, PoseOptimization = 7) the local BA landed on the
// queue of an extractor in about one process out of three: 0.79 instead of 0.59 ms per solve and 5600 instead of 8400 frames/s for
// the whole run, same cores, no host noise.  The library therefore owns FOUR non-blocking streams per device,
// created together by the first handle so that each gets a hardware queue of its own:
//   "lba"                              -> L        (local BA handles; nothing else ever)
//   "ex"                               -> E0 / E1  (extractor handles, alternating: Frame(t+1) is built next to the searches on frame t)
//   "fr"                               -> M in a process that has extractors (a frame built by the constructor is on its extractor's
//                                         stream until that constructor has been collected, then back on M: matcher.hip,
//                                         orbm_internal_set_n); M, E0, E1 in turn in a process without (the server's KeyFrame matchers)
//   "map", "po", "bow", "db", "misc"   -> M        (map uploads, PoseOptimization, vocabulary / database work, stand-alone utilities)
// None of them is the legacy null stream: nothing the library launches joins (or is joined by) the blocking streams of the
// application it is embedded in.  An application that itself keeps streams busy should run with GPU_MAX_HW_QUEUES >= 4 + its own
// (include/orbgpu.h, "Streams"), or hand the library its streams: every handle type has a *_set_stream entry point.
// Handles that share a stream stay correct -- every completion signal is enqueued behind the handle's own work on an in-order
// stream -- they merely do not overlap.  ORBG_STREAM_POOL=0 gives every handle a stream of its own again.  Implemented in misc.cpp
// (one registry for all translation units).
hipError_t create_stream(hipStream_t* st, const char* role);
void release_stream(hipStream_t st);       // destroys a stream of its own; pool streams live as long as the process
bool is_library_stream(hipStream_t st);    // one of the pool's streams (shared between handles: never capture on it, never destroy it)

inline int select_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return ORBG_NO_DEVICE;
  if (device < 0 || device >= n) return ORBG_BAD_ARG;
  ORBG_HIP(hipSetDevice(device));
  return ORBG_OK;
}

// *_set_stream (include/orbgpu.h, "Streams"): the handle's work goes to the caller's stream from now on; NULL = back to the library's
// stream of the role.  The handle must be idle; its old stream is drained first.  A caller's stream is never destroyed by the library.
inline int swap_stream(hipStream_t* slot, bool* external, void* user, const char* role) {
  if (*slot) ORBG_HIP(hipStreamSynchronize(*slot));
  if (!*external) release_stream(*slot);
  *slot = nullptr;
  if (user) { *slot = (hipStream_t)user; *external = true; }
  else { *external = false; ORBG_HIP(create_stream(slot, role)); }
  return ORBG_OK;
}

// the M stream of the current device for a stand-alone utility call (a stream of its own, destroyed on scope exit, when the pool is off)
struct MiscStream {
  hipStream_t s = nullptr;
  int open() { ORBG_HIP(create_stream(&s, "misc")); return ORBG_OK; }
  ~MiscStream() { if (s) { (void)hipStreamSynchronize(s); release_stream(s); } }
};

// for a call on a KEPT stream that copies into the caller's memory: however the scope is left, an error return included, nothing it
// enqueued is still in flight afterwards (MiscStream does the same for its per-call stream)
struct StreamDrain {
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// how many owners of an eight-workgroup LDL^T context (ldlt_solver.hpp) this process has had before the caller: each takes another XCD
int next_ldlt_xcd_user();

// Phase timing of a solve (ba_set_profiling, eg_set_profiling): event pairs around launch groups, read at the next synchronisation;
// ms[phase] sums them.  While `on` is false (and before the first reset() with it true) no member makes a HIP call.
template <int N>
struct PhaseTimer {
  bool on = false;
  double ms[N] = {};
  hipEvent_t ev[32] = {};
  int ev_phase[16] = {};
  int ev_n = 0;
  // the start of a solve: zeroed sums, the events created on first use
  int reset() {
    if (!on) return ORBG_OK;
    for (double& m : ms) m = 0;
    ev_n = 0;
    for (hipEvent_t& e : ev) if (!e) ORBG_HIP(hipEventCreate(&e));
    return ORBG_OK;
  }
  void begin(int phase, hipStream_t st) {
    if (!on) return;
    if (ev_n == 16) flush(st);
    if (hipEventRecord(ev[2 * ev_n], st) == hipSuccess) ev_phase[ev_n] = phase;
  }
  void end(hipStream_t st) {
    if (!on) return;
    if (hipEventRecord(ev[2 * ev_n + 1], st) == hipSuccess) ev_n++;
  }
  void flush(hipStream_t st) {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    for (int i = 0; i < ev_n; i++) {
      float t = 0;
      if (hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) ms[ev_phase[i]] += t;
    }
    ev_n = 0;
  }
  void release() { for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
};

// The work area of an entry point WITHOUT a handle (pose_optimize, orbm_sim3_solve_batch, ...: the reference calls a static member, so
// the buffers belong to the calling thread: `static thread_local WorkArea<...>`), also the device half of a small handle.  Bufs holds
// the site's buffers and `void release_buffers()`; the area adds the device they live on and the stream the calls run on.  It derives
// FROM the buffers so that they are still alive when its destructor -- thread exit for a thread_local -- releases them.
template <class Bufs>
struct WorkArea : Bufs {
  int device = -1;
  hipStream_t stream = nullptr;
  bool ext_stream = false;                 // `stream` is the caller's (swap_stream): never destroyed here
  WorkArea() = default;
  WorkArea(const WorkArea&) = delete;
  WorkArea& operator=(const WorkArea&) = delete;
  // selects `dev`; what the area holds on another device is released first; the stream of `role` is created on first use
  int open(int dev, const char* role) {
    int rc = select_device(dev);
    if (rc) return rc;
    if (device != dev) { release(); device = dev; }
    if (!stream) { ORBG_HIP(create_stream(&stream, role)); ext_stream = false; }
    return ORBG_OK;
  }
  // on the device the buffers live on, after the stream has drained.  Errors are swallowed: this also runs at thread and process exit.
  void release() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    if (stream) { (void)hipStreamSynchronize(stream); if (!ext_stream) release_stream(stream); stream = nullptr; }
    ext_stream = false;
    Bufs::release_buffers();
    device = -1;
  }
  ~WorkArea() { release(); }
};

}  // namespace orbg
