// The library's own replay (multi_orbslam3_amd/csrc/init_replay.hpp) as a stand-alone host program: a CPU test builds it with
// -fsanitize=address,undefined, feeds it the candidate lists of tests/search_init_model.py and compares what it prints with the model.
//   init_replay_check <lists.bin>
//   init_replay_check <lists.bin> <reps>    median time of the replay alone, in microseconds (tools/search_init_time.py, built -O2)
// lists.bin: int32 n1, n2, check_orientation; float nn_ratio; list_start (n1 + 1 int32); entries (list_start[n1] uint32); octave1
// (n1 int32); angle1 (n1 float); angle2 (n2 float); pt2 (n2 x 2 float); prev (n1 x 2 float).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "init_replay.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[3]; float nn;
  if (std::fread(h, 4, 3, f) != 3 || std::fread(&nn, 4, 1, f) != 1 || h[0] < 0 || h[1] < 0) return 2;
  const int n1 = h[0], n2 = h[1];
  std::vector<int32_t> start, octave; std::vector<uint32_t> entries; std::vector<float> a1, a2, pt2, prev;
  if (!rd(f, start, (size_t)n1 + 1) || !rd(f, entries, (size_t)start[n1]) || !rd(f, octave, n1) || !rd(f, a1, n1) || !rd(f, a2, n2) ||
      !rd(f, pt2, 2 * (size_t)n2) || !rd(f, prev, 2 * (size_t)n1)) return 2;
  std::fclose(f);
  std::vector<int32_t> base(n1), count(n1), m12(n1);
  for (int i = 0; i < n1; i++) { base[i] = start[i]; count[i] = octave[i] > 0 ? -1 : start[i + 1] - start[i]; }
  orbg::InitReplayScratch S; orbg::InitReplayCounters C;
  if (argc > 2) {
    std::vector<double> us;
    for (int r = std::atoi(argv[2]); r > 0; r--) {
      std::vector<float> p = prev;
      const auto t0 = std::chrono::steady_clock::now();
      orbg::init_search_replay(n1, n2, base.data(), count.data(), entries.data(), a1.data(), a2.data(), pt2.data(), nn, h[2] != 0, p.data(),
                               m12.data(), S, &C);
      us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    std::printf("replay_us_median %.1f\n", us.empty() ? 0.0 : us[us.size() / 2]);
    return 0;
  }
  const int n = orbg::init_search_replay(n1, n2, base.data(), count.data(), entries.data(), a1.data(), a2.data(), pt2.data(), nn, h[2] != 0,
                                         prev.data(), m12.data(), S, &C);
  std::printf("nmatches %d\ncounters %d %d %d %d\nmatches12:", n, C.n_queries, C.n_candidates, C.n_evictions, C.n_rot_rejected);
  for (int i = 0; i < n1; i++) std::printf(" %d", m12[i]);
  std::printf("\nprev:");
  for (size_t i = 0; i < prev.size(); i++) { uint32_t u; std::memcpy(&u, &prev[i], 4); std::printf(" %08x", u); }
  std::printf("\n");
  return 0;
}
