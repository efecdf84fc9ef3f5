// csrc/stage_layout.hpp under seeded random slot sequences (host only; built by tests/test_adapters_cpp.py with
// g++ -fsanitize=address,undefined): every offset a multiple of 16, no two slots overlap, the total covers the last slot, the bound
// never below the total reached.  One sequence passes 4 GiB (arithmetic only: nothing is allocated).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/orbgpu.h"
#include "../../multi_orbslam3_amd/csrc/stage_layout.hpp"

using orbg::StageLayout;

namespace {

// elements of 12, 16 and 32 bytes, and stand-ins with the sizes of the device-side records that no public header declares (the
// pose-optimisation output record, a Sim3 job descriptor); the public record structs are staged as themselves
struct Rec12 { float f[3]; };
struct alignas(16) Rec16 { char b[16]; };
struct Rec32 { double d[4]; };
struct Rec120 { double d[15]; };
struct Rec200 { double d[25]; };

struct Span { size_t off, end; };
int g_fail = 0;

void fail(const char* what, int seq, size_t i) {
  if (g_fail++ < 10) printf("FAIL %s: sequence %d, slot %zu\n", what, seq, i);
}

template <typename T>
void add(StageLayout& lay, size_t count, std::vector<Span>& spans, size_t& payload) {
  const orbg::StageSlot<T> s = lay.add<T>(count);
  if (s.count != count || s.bytes() != count * sizeof(T) || s.end() != s.off + s.bytes()) g_fail++;
  spans.push_back(Span{s.off, s.end()});
  payload += s.bytes();
}

void add_kind(int kind, StageLayout& lay, size_t count, std::vector<Span>& spans, size_t& payload) {
  switch (kind) {
    case 0: add<uint8_t>(lay, count, spans, payload); break;
    case 1: add<uint16_t>(lay, count, spans, payload); break;
    case 2: add<float>(lay, count, spans, payload); break;
    case 3: add<double>(lay, count, spans, payload); break;
    case 4: add<Rec12>(lay, count, spans, payload); break;
    case 5: add<Rec16>(lay, count, spans, payload); break;
    case 6: add<Rec32>(lay, count, spans, payload); break;
    case 7: add<Rec120>(lay, count, spans, payload); break;
    case 8: add<Rec200>(lay, count, spans, payload); break;
    case 9: add<orbx_keypoint>(lay, count, spans, payload); break;
    case 10: add<orbm_fuse_record>(lay, count, spans, payload); break;
    default: add<orbm_newpoints_record>(lay, count, spans, payload);
  }
}

void check(const StageLayout& lay, const std::vector<Span>& spans, size_t payload, int seq) {
  size_t prev_end = 0;
  for (size_t i = 0; i < spans.size(); i++) {
    if (spans[i].off % 16) fail("offset not a multiple of 16", seq, i);
    if (spans[i].off < prev_end) fail("slot overlaps its predecessor", seq, i);     // (slots come in ascending order)
    if (spans[i].end < spans[i].off) fail("slot wraps", seq, i);
    prev_end = spans[i].end;
  }
  if (lay.bytes() < prev_end || lay.bytes() % 16) fail("total does not cover the last slot", seq, spans.size());
  if (StageLayout::bound(spans.size(), payload) < lay.bytes()) fail("bound below the total", seq, spans.size());
}

}  // namespace

int main() {
  static_assert(sizeof(Rec12) == 12 && sizeof(Rec16) == 16 && sizeof(Rec32) == 32 && sizeof(Rec120) == 120 && sizeof(Rec200) == 200, "record sizes");
  std::mt19937 rng(20251);
  int n_seq = 0;
  size_t residues_seen = 0;
  for (int seq = 0; seq < 4000; seq++, n_seq++) {
    StageLayout lay;
    std::vector<Span> spans;
    size_t payload = 0;
    const int k = 1 + (int)(rng() % 24);
    for (int i = 0; i < k; i++) {
      const int kind = (int)(rng() % 12);
      const unsigned pick = rng() % 8;
      const size_t count = pick == 0 ? 0 : pick == 1 ? 1 : pick < 6 ? rng() % 40 : rng() % 5000;
      add_kind(kind, lay, count, spans, payload);
      residues_seen |= (size_t)1 << (lay.end % 16);
    }
    check(lay, spans, payload, seq);
  }
  // byte slots whose ends visit every residue mod 16, each followed by a zero-count slot (which takes nothing beyond alignment)
  for (size_t r = 0; r < 16; r++, n_seq++) {
    StageLayout lay;
    std::vector<Span> spans;
    size_t payload = 0;
    add<uint8_t>(lay, 32 + r, spans, payload);
    residues_seen |= (size_t)1 << (lay.end % 16);
    const size_t before = lay.bytes();
    add<double>(lay, 0, spans, payload);
    if (lay.bytes() != before) fail("an empty slot consumed bytes", 100000 + (int)r, 1);
    add<Rec120>(lay, 3, spans, payload);
    check(lay, spans, payload, 100000 + (int)r);
  }
  if (residues_seen != 0xFFFF) { printf("FAIL: section ends did not reach every residue mod 16 (%zx)\n", residues_seen); g_fail++; }
  {                                         // past 4 GiB: offsets are size_t all the way
    StageLayout lay;
    std::vector<Span> spans;
    size_t payload = 0;
    for (int i = 0; i < 6; i++) {
      add<Rec12>(lay, ((size_t)1 << 27) + 5, spans, payload);     // 1.5 GiB + 60 bytes each
      add<uint8_t>(lay, 7, spans, payload);
    }
    check(lay, spans, payload, 200000);
    if (lay.bytes() <= ((size_t)1 << 32) || spans.back().off <= ((size_t)1 << 32)) fail("the long sequence stayed below 4 GiB", 200000, 0);
    n_seq++;
  }
  if (g_fail) { printf("%d failures\n", g_fail); return 1; }
  printf("%d slot sequences checked: ALL OK\n", n_seq);
  return 0;
}
