// Layout of a staging block: typed slots at 16-byte-aligned offsets, handed out by a bump allocator.  Host-only arithmetic (no HIP
// header: tests/cpp/stage_layout_check.cpp builds it with plain g++).  The ONLY place in the library that rounds a staging offset;
// StageBlock (common.hpp) turns a slot into a pointer.
#pragma once

#include <cstddef>

namespace orbg {

// `count` elements of T at byte offset `off` of a block.  count == 0 is legal: the slot has an offset and no bytes.
template <typename T>
struct StageSlot {
  size_t off = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
  size_t end() const { return off + bytes(); }
};

struct StageLayout {
  static constexpr size_t kAlign = 16;    // every section may hold double / u64 / uint4: one rule for all of them
  static constexpr size_t round_up(size_t x) { return (x + (kAlign - 1)) & ~(kAlign - 1); }
  size_t end = 0;                         // end of the last slot's payload
  template <typename T>
  StageSlot<T> add(size_t count) {
    static_assert(alignof(T) <= kAlign, "a staged type wants more than the block's alignment");
    StageSlot<T> s{round_up(end), count};
    end = s.end();
    return s;
  }
  size_t bytes() const { return round_up(end); }     // the block's size: covers the last slot, whole 16-byte words (copy kernels move uint4)
  // upper bound of bytes() after `slots` slots holding `payload` bytes between them, in any order: each slot pads at most 15 bytes
  static constexpr size_t bound(size_t slots, size_t payload) { return payload + kAlign * slots; }
};

}  // namespace orbg
