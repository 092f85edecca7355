// wbc_entry_in.h — which optional input lane s of a packed sim3 row fetches at the kernel's entry (wbc_k_sim3p.hip): the array, the
// element offset inside it and whether the lane fetches at all, for instance b and the set of arrays the caller passed. The kernel turns the answer
// into ONE predicated load per lane (the array's base pointer chosen by selects) in place of nested if / else arms with a load each, so that every
// input of the instance leaves in the same memory level. No device or HIP header is needed: a plain host compiler can include this file
// (tests/test_sim3p_entry_host.py checks every lane, every presence mask and both ends of a batch against the arms this replaces).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WBC_ENTRY_FN __host__ __device__ __forceinline__
#else
#define WBC_ENTRY_FN static inline
#endif

namespace wbc {

// the optional input arrays of WbcTickIn the entry reads, and their row lengths (doubles per instance)
enum : int { EIN_EE_TARGET = 0, EIN_PREV_EE_TARGET = 1, EIN_TRUNK_BOX_CENTER = 2, EIN_EE_REF_ROT = 3, EIN_COUNT = 4 };   // (EE_REF_ROT: ee_prev_rot goes with it)
constexpr int EIN_ROW[EIN_COUNT] = {15, 15, 4, 45};

struct EntryIn {
  int arr;          // EIN_*: the array the lane would read
  int64_t off;      // element offset inside it
  bool on;          // the lane reads (the array is present and the lane has an entry of it); off lanes stay masked off
};

// presence mask: bit EIN_x set = the caller passed array x
// Lane s's extra input `ex` -> V.in[28 + s]: the gripper's target position (lanes 0..2: ee_target[b][12 + s]), its previous value (lanes 3..5:
// prev_ee_target[b][12 + (s - 3)]), the trunk box's centre (lanes 6..9: trunk_box_center[b][s - 6]); lanes 10..15 have none.
WBC_ENTRY_FN EntryIn entry_in_ex(const int s, const int64_t b, const unsigned present) {
  EntryIn e;
  e.arr = s < 3 ? EIN_EE_TARGET : (s < 6 ? EIN_PREV_EE_TARGET : EIN_TRUNK_BOX_CENTER);
  const int row = s < 6 ? 15 : 4, col = s < 3 ? 12 + s : (s < 6 ? 12 + (s - 3) : s - 6);   // (selects on small integers, one multiply)
  e.off = b * row + col;
  e.on = s < 10 && ((present >> e.arr) & 1u);
  return e;
}
// Lane s's entry of the gripper's orientation reference (and of its previous value, same offset in ee_prev_rot): ee_ref_rot[b][36 + s], lanes 0..8
WBC_ENTRY_FN EntryIn entry_in_rot(const int s, const int64_t b, const unsigned present) {
  EntryIn e;
  e.arr = EIN_EE_REF_ROT;
  e.off = b * 45 + 36 + s;
  e.on = s < 9 && ((present >> EIN_EE_REF_ROT) & 1u);
  return e;
}

}  // namespace wbc
