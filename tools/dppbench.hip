// dppbench — what a 16-lane row broadcast costs as one v_mov_b64_dpp row_newbcast (wbc_packed.h row_bc) against the store + ds_read_b128 round trip
// it replaces in the packed sim3 tick. One kernel, four bodies, timed per wave with clock64 over REPS trips of 12 values:
//   chain   12 dependent (row_bc -> v_fma_f64) pairs: the move's result latency, once the fma-only chain is taken off
//   fma     12 dependent v_fma_f64 alone: that baseline
//   block   12 independent row_bc of one value (+ one fma that makes the next trip depend on this one): the move's issue cost
//   lds     one 8-byte store per lane, six ds_read_b128 of the row's vector, one fma on the last value read: the LDS round trip
// Run as a lone wave and as 8 waves per CU on every CU (the tick's occupancy: 20 288 B of LDS per wave); prints cycles per trip, mean over waves.
//   hipcc --offload-arch=gfx950 -O3 dppbench.hip -o build/dppbench && build/dppbench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <utility>
#include <vector>
template <int K>
__device__ __forceinline__ double row_bc(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + K, 0xF, 0xF, true); }
template <int... K>
__device__ __forceinline__ double chain(double v, const double c, const double d, std::integer_sequence<int, K...>) {
  ((v = fma(row_bc<K>(v), c, d)), ...);
  return v;
}
template <int... K>
__device__ __forceinline__ double fmas(double v, const double c, const double d, std::integer_sequence<int, K...>) {
  (((void)K, v = fma(v, c, d)), ...);
  return v;
}
__device__ __forceinline__ void keep(const double x) { asm volatile("" ::"v"(x)); }
template <int... K>
__device__ __forceinline__ void block(const double v, std::integer_sequence<int, K...>) {
  double b[sizeof...(K)];
  ((b[K] = row_bc<K>(v)), ...);
  (keep(b[K]), ...);
}
constexpr int NV = 12;
enum { CHAIN, FMA, BLOCK, LDS };
template <int MODE>
__global__ void __launch_bounds__(64) k_bench(double* __restrict__ sink, long long* __restrict__ cyc, const int reps, const double c, const double d) {
  extern __shared__ double lds[];           // (one wave per block: entries 0..63 are used, the rest sets the occupancy)
  const int lane = threadIdx.x, row = lane & 48;
  double v = 1.0 + 1e-3 * lane;
  lds[lane] = v;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_sched_barrier(0);
  const long long t0 = clock64();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
  for (int i = 0; i < reps; ++i) {
    if (MODE == CHAIN) v = chain(v, c, d, std::make_integer_sequence<int, NV>());
    if (MODE == FMA) v = fmas(v, c, d, std::make_integer_sequence<int, NV>());
    if (MODE == BLOCK) { block(v, std::make_integer_sequence<int, NV>()); v = fma(v, c, d); }
    if (MODE == LDS) {
      lds[lane] = v;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      double2 b[NV / 2];
#pragma unroll
      for (int k = 0; k < NV / 2; ++k) b[k] = *reinterpret_cast<const double2*>(lds + row + 2 * k);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
      for (int k = 0; k < NV / 2; ++k) { keep(b[k].x); keep(b[k].y); }
      v = fma(b[NV / 2 - 1].y, c, d);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  const long long t1 = clock64();
  __builtin_amdgcn_sched_barrier(0);
  sink[(size_t)blockIdx.x * 64 + lane] = v;
  if (lane == 0) cyc[blockIdx.x] = t1 - t0;
}
template <int MODE>
static void run(double* sink, long long* cyc, const int grid, const size_t ldsb, const int reps, const char* what) {
  std::vector<long long> h(grid);
  for (int i = 0; i < 2; ++i) hipLaunchKernelGGL((k_bench<MODE>), dim3(grid), dim3(64), ldsb, 0, sink, cyc, reps, 0.999, 1e-3);
  if (hipMemcpy(h.data(), cyc, grid * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: failed\n", what); exit(1); }
  double mean = 0.0; long long lo = h[0], hi = h[0];
  for (long long x : h) { mean += (double)x; lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
  mean /= grid;
  printf("%-7s waves %5d  LDS %6zu B  cycles per trip of %d: mean %8.1f  (min %.1f max %.1f)  per value %.2f\n", what, grid, ldsb, NV, mean / reps,
         (double)lo / reps, (double)hi / reps, mean / reps / NV);
}
int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
  const int full = 8 * p.multiProcessorCount, reps = 2000;
  double* sink; long long* cyc;
  if (hipMalloc(&sink, (size_t)full * 64 * 8) != hipSuccess || hipMalloc(&cyc, (size_t)full * 8) != hipSuccess) { printf("no memory\n"); return 1; }
  for (int grid : {1, full}) {
    const size_t ldsb = 20288;
    run<CHAIN>(sink, cyc, grid, ldsb, reps, "chain");
    run<FMA>(sink, cyc, grid, ldsb, reps, "fma");
    run<BLOCK>(sink, cyc, grid, ldsb, reps, "block");
    run<LDS>(sink, cyc, grid, ldsb, reps, "lds");
  }
  return 0;
}
