// wbc_wave_geom.h — the slice geometry of the packed sim3 kernel's wave order (wbc_device.h WaveOrder, wbc_packed.h wo_*)
// as launch constants: the host knows the grid, so it works out once per launch what every wave used to derive with three signed 32-bit
// divisions by ns. No device or HIP header is needed: a plain host compiler can include this file (tests/test_wave_geom.py does).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WBC_GEOM_FN __host__ __device__ __forceinline__
#else
#define WBC_GEOM_FN static inline
#endif

namespace wbc {

constexpr uint32_t WO_GEOM_SW = 127;       // waves per slice at most (wbc_device.h WO_SW; checked there)
constexpr uint32_t WO_GEOM_XMAX = (1u << 17) + 256u;   // the reciprocal is exact for every x below this and every 1 <= ns <= 256

// Wave grp of a launch of `waves` waves is wave k = grp / ns of slice g = grp % ns, ns = ceil(waves / 127). The kernel's one extra parameter:
struct WoGeom {
  uint32_t ns;       // slices of the launch
  uint32_t magic;    // ceil(2^32 / ns) for ns >= 2: x / ns == umulhi(x, magic) for x < WO_GEOM_XMAX, ns <= 256; 0 for ns == 1 (2^32 does not fit: x / 1 = x)
  uint32_t wq, wr;   // waves / ns and waves % ns: slice g holds wq + (g < wr) waves, and the launch's last wave sits in slice (wr ? wr : ns) - 1
};

WBC_GEOM_FN WoGeom wo_geom(const uint32_t waves) {
  WoGeom w;
  w.ns = (waves + WO_GEOM_SW - 1u) / WO_GEOM_SW;
  if (w.ns == 0u) w.ns = 1u;
  // floor(2^32 / ns) + 1: with e = magic ns - 2^32 in (0, ns], umulhi(x, magic) = floor(x / ns + x e / (ns 2^32)) is floor(x / ns) while x e < 2^32
  // (the fraction of x / ns is at most 1 - 1 / ns) — x < 2^17 + 256 and e <= ns <= 256 stay 2^7 below that
  w.magic = w.ns >= 2u ? (uint32_t)(0x100000000ull / w.ns) + 1u : 0u;
  w.wq = waves / w.ns;
  w.wr = waves % w.ns;
  return w;
}
// x / ns and x % ns (x < WO_GEOM_XMAX, ns <= 256): one multiply-high, one multiply, one subtraction
WBC_GEOM_FN uint32_t wo_div(const WoGeom& w, const uint32_t x) {
  return w.ns == 1u ? x : (uint32_t)(((uint64_t)x * w.magic) >> 32);
}
WBC_GEOM_FN uint32_t wo_mod(const WoGeom& w, const uint32_t x, const uint32_t k) { return x - k * w.ns; }   // k = wo_div(w, x)

}  // namespace wbc
