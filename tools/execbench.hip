// execbench — what one per-lane exec-mask region (v_cmp, s_and_saveexec_b64, s_cbranch_execz, body, s_or_b64 exec) costs a wave of the packed sim3
// tick against the same work done on all lanes and selected. One kernel per form, timed per wave with clock64 over REPS trips of a
// chain of 32 steps; step I guards with `s < K_I` (K_I = 1 + 7 I mod 15: a different compile-time bound every step, so no two regions merge), s the
// lane of the 16-lane row, and carries the chain on with one v_fma_f64 (the loads feed it, the stores do not):
//   fma       32 dependent v_fma_f64 alone: the baseline every other form contains
//   st_if     (a) if (s < K) ds_write_b64 of the chain value to the row's vector
//   st_sel    (b) the same store unconditional, to (s < K) ? its address : the row's 16-byte dump slot
//   st_few    (f) as st_sel with K = 1 .. 3: thirteen or more lanes of every row write the row's dump slot — do same-address writes serialise?
//   ld_if     (c) x = 0; if (s < K) x = ds_read_b64 (dynamic LDS: the compiler cannot speculate the load)
//   ld_sel    (d) ds_read_b64 from an address clamped into the row's vector on every lane, then v_cndmask
//   fma6_if   (e) if (s < K) a block of six dependent v_fma_f64 (kept a region: an empty volatile asm inside), else 0
//   fma6_sel  (e) the six on all lanes, then v_cndmask
// Run as a lone wave and as 8 waves per CU on every CU (the tick's occupancy: 20 288 B of LDS per wave). Prints cycles per trip (mean over waves) and,
// per step, what the form adds to the fma baseline.
//   hipcc --offload-arch=gfx950 -O3 execbench.hip -o build/execbench && build/execbench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
enum { FMA, ST_IF, ST_SEL, ST_FEW, LD_IF, LD_SEL, FMA6_IF, FMA6_SEL };
constexpr int NSTEP = 32;
constexpr int LDS_ROWS = 64, LDS_DUMP = 64;   // doubles: the four rows' vectors [16] at 16 r, the rows' dump slots [2] at 64 + 2 r
template <int MODE, int I>
__device__ __forceinline__ void step(double& v, double* const lds, const int r, const int s, const double c, const double d) {
  constexpr int K = (MODE == ST_FEW) ? 1 + I % 3 : 1 + (I * 7) % 15;
  double* const row = lds + 16 * r;
  double* const dump = lds + LDS_DUMP + 2 * r;
  if (MODE == ST_IF) { if (s < K) row[s] = v; }
  if (MODE == ST_SEL || MODE == ST_FEW) { double* const p = (s < K) ? row + s : dump; *p = v; }
  double x = d;
  if (MODE == LD_IF) { x = 0.0; if (s < K) x = lds[(16 * r + s + I) & (LDS_ROWS - 1)]; }
  if (MODE == LD_SEL) { const double y = lds[(16 * r + min(s, K - 1) + I) & (LDS_ROWS - 1)]; x = (s < K) ? y : 0.0; }
  if (MODE == FMA6_IF) {
    x = 0.0;
    if (s < K) {
      double t = v;
#pragma unroll
      for (int k = 0; k < 6; ++k) t = fma(t, c, d);
      asm volatile("" : "+v"(t));
      x = t;
    }
  }
  if (MODE == FMA6_SEL) {
    double t = v;
#pragma unroll
    for (int k = 0; k < 6; ++k) t = fma(t, c, d);
    x = (s < K) ? t : 0.0;
  }
  v = fma(v, c, x);
  asm volatile("" : "+v"(v));     // (the steps stay 32 steps)
}
template <int MODE, int... I>
__device__ __forceinline__ void chain(double& v, double* const lds, const int r, const int s, const double c, const double d, std::integer_sequence<int, I...>) {
  (step<MODE, I>(v, lds, r, s, c, d), ...);
}
template <int MODE>
__global__ void __launch_bounds__(64) k_bench(double* __restrict__ sink, long long* __restrict__ cyc, const int reps, const double c, const double d) {
  extern __shared__ double lds[];           // (one wave per block: entries 0 .. 71 are used, the rest sets the occupancy)
  const int lane = threadIdx.x, r = lane >> 4, s = lane & 15;
  double v = 1.0 + 1e-3 * lane;
  lds[lane] = v;
  if (lane < 8) lds[LDS_DUMP + lane] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_sched_barrier(0);
  const long long t0 = clock64();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
  for (int i = 0; i < reps; ++i) chain<MODE>(v, lds, r, s, c, d, std::make_integer_sequence<int, NSTEP>());
  __builtin_amdgcn_sched_barrier(0);
  const long long t1 = clock64();
  __builtin_amdgcn_sched_barrier(0);
  sink[(size_t)blockIdx.x * 64 + lane] = v + lds[lane] + lds[LDS_DUMP + (lane & 7)];
  if (lane == 0) cyc[blockIdx.x] = t1 - t0;
}
template <int MODE>
static double run(double* sink, long long* cyc, const int grid, const size_t ldsb, const int reps, const char* what, const double base) {
  std::vector<long long> h(grid);
  for (int i = 0; i < 2; ++i) hipLaunchKernelGGL((k_bench<MODE>), dim3(grid), dim3(64), ldsb, 0, sink, cyc, reps, 0.999, 1e-3);
  if (hipMemcpy(h.data(), cyc, grid * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: failed\n", what); exit(1); }
  double mean = 0.0; long long lo = h[0], hi = h[0];
  for (long long x : h) { mean += (double)x; lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
  mean /= grid;
  printf("%-9s waves %5d  cycles per trip of %d steps: mean %8.1f  (min %.1f max %.1f)  per step %6.2f  over fma %+6.2f\n", what, grid, NSTEP, mean / reps,
         (double)lo / reps, (double)hi / reps, mean / reps / NSTEP, base < 0.0 ? 0.0 : (mean / reps - base) / NSTEP);
  return mean / reps;
}
int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
  const int full = 8 * p.multiProcessorCount, reps = 1000;
  double* sink; long long* cyc;
  if (hipMalloc(&sink, (size_t)full * 64 * 8) != hipSuccess || hipMalloc(&cyc, (size_t)full * 8) != hipSuccess) { printf("no memory\n"); return 1; }
  for (int grid : {1, full}) {
    const size_t ldsb = 20288;
    const double base = run<FMA>(sink, cyc, grid, ldsb, reps, "fma", -1.0);
    run<ST_IF>(sink, cyc, grid, ldsb, reps, "st_if", base);
    run<ST_SEL>(sink, cyc, grid, ldsb, reps, "st_sel", base);
    run<ST_FEW>(sink, cyc, grid, ldsb, reps, "st_few", base);
    run<LD_IF>(sink, cyc, grid, ldsb, reps, "ld_if", base);
    run<LD_SEL>(sink, cyc, grid, ldsb, reps, "ld_sel", base);
    run<FMA6_IF>(sink, cyc, grid, ldsb, reps, "fma6_if", base);
    run<FMA6_SEL>(sink, cyc, grid, ldsb, reps, "fma6_sel", base);
  }
  return 0;
}
