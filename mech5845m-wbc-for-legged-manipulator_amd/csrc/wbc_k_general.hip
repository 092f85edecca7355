// wbc_k_general.hip — the general tick kernel wbc_tick_kernel<MODE, WARM, ORTH> (one instance per wavefront; tick / assemble / FK outputs).
#include "wbc_common.h"

namespace wbc {

// ------------------------------------------------------------------------------------------------
// kernels: single-wave workgroups, one per instance for the tick kernels (the QP / integrate kernels walk the batch with a
// grid-stride loop whose exit, b >= B, every wave reaches).
// ------------------------------------------------------------------------------------------------
// WARM: the variant that reads / writes working sets (warm start, KernelArgs.ws_in / ws_out); the cold variant carries none of it
// ORTH: the variant that carries contact_presolve_orth (chosen by launch_tick when a plan of the batch asks for it: the other
// variants keep their register allocation — with the extra code inlined the general kernel went from 198 VGPRs to 256 + spills)
// ROT: rotated joint placements in the handle (KernelArgs.rot, fk_levels)
template <int MODE, bool WARM = false, bool ORTH = false, bool ROT = false>
__global__ void __launch_bounds__(64, 2) wbc_tick_kernel(const KernelArgs A, const DevModel* __restrict__ models,
                                                         const WbcConfig* __restrict__ cfgs, const DevPlan* __restrict__ plans) {
  // models / cfgs are separate __restrict__ const parameters so that the compiler may read them with scalar loads
  // (as members of A it must assume the kernel's own stores clobber them: every access became a vector load + full wait).
  // ONE instance per single-wave workgroup, no loop: inside a persistent loop the compiler hoists hundreds of
  // "invariants" (polynomial coefficients, masks, addresses) out of the tick, spills them to scratch and reloads them
  // one by one with full memory waits (profiles/r01_phase_cycles_v6: 60k cycles in one atan2). The hardware's
  // workgroup dispatcher does the batch loop instead; other resident waves cover this wave's input latency.
  __shared__ Smem S;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
#ifdef WBC_PROFILE
  const unsigned long long t_entry = clock64();
#else
  const unsigned long long t_entry = 0;
#endif
  S.cl[lane] = 0.0;                            // zero padding (never written above entry 25)
  const bool has2 = A.in.trunk_target || A.in.prev_trunk_target || A.in.trunk_ref_euler || A.in.trunk_prev_rot ||
                    A.in.com_target || A.in.com_target_vel;
  const bool has3 = A.in.ee_ref_rot != nullptr;
  // the model index is wave-uniform: say so, or every M.* / cfg.* access becomes a vector load
  const int mid = model_index(A.in.model_id, b, A.n_models);
  const InRegs cur = load_inputs(A.in, A.dbg_alias ? 0 : b, lane, has2, has3);   // dbg_alias: diagnostic, every wave reads instance 0
  const LaneConst lc = load_lane_const(models[mid], cfgs[mid], lane);   // L1/L2-resident 3 KB table
  stage_inputs(S, cur, lane, has2, has3);
  WSYNC();
  process_instance<MODE, WARM, ORTH, ROT>(S, A, models[mid], cfgs[mid], plans[mid], lc, cur, b, lane, t_entry);
}

// TP: the same tick with per-instance weights and gains (tp [B], wbc_tick_tp / wbc_assemble_tp): row b replaces cfgs[mid]'s weight / gain
// block (a row that tp_row_bad refuses gives the instance WBC_QP_NUMERICAL). A kernel of its own, so that the kernels above keep their code.
template <int MODE, bool WARM = false, bool ORTH = false, bool ROT = false>
__global__ void __launch_bounds__(64, 2) wbc_tick_tp_kernel(const KernelArgs A, const DevModel* __restrict__ models,
                                                            const WbcConfig* __restrict__ cfgs, const DevPlan* __restrict__ plans,
                                                            const WbcTaskParams* __restrict__ tp) {
  __shared__ Smem S;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  S.cl[lane] = 0.0;
  const bool has2 = A.in.trunk_target || A.in.prev_trunk_target || A.in.trunk_ref_euler || A.in.trunk_prev_rot ||
                    A.in.com_target || A.in.com_target_vel;
  const bool has3 = A.in.ee_ref_rot != nullptr;
  const int mid = model_index(A.in.model_id, b, A.n_models);
  const InRegs cur = load_inputs(A.in, A.dbg_alias ? 0 : b, lane, has2, has3);
  const LaneConst lc = load_lane_const(models[mid], cfgs[mid], lane);
  // (an assembly reports no status: its rows enter as they are)
  const bool tp_bad = MODE == MODE_TICK && tp_row_bad(tp + b, lane);
  const TpRow tpr = tp_bad ? (TpRow)&cfgs[mid].ee_W[0][0] : (TpRow)(tp + b);
  stage_inputs(S, cur, lane, has2, has3);
  WSYNC();
  process_instance<MODE, WARM, ORTH, ROT, true>(S, A, models[mid], cfgs[mid], plans[mid], lc, cur, b, lane, 0ull, tpr, tp_bad);
}

// One translation unit per PART (csrc/Makefile compiles this file once per part, in parallel): each part instantiates some of the kernel's
// variants; part 0 also holds the launcher and sees the other parts' variants as explicit-instantiation declarations.
#ifndef GENERAL_PART
#define GENERAL_PART -1      // -1: everything in one unit
#endif
#define KINST(...) template __global__ void wbc_tick_kernel<__VA_ARGS__>(const KernelArgs, const DevModel* __restrict__, const WbcConfig* __restrict__, const DevPlan* __restrict__);
#define KDECL(...) extern template __global__ void wbc_tick_kernel<__VA_ARGS__>(const KernelArgs, const DevModel* __restrict__, const WbcConfig* __restrict__, const DevPlan* __restrict__);
#if GENERAL_PART == 0 || GENERAL_PART == -1
KINST(MODE_TICK)
#endif
#if GENERAL_PART == 1 || GENERAL_PART == -1
KINST(MODE_TICK, true)
#elif GENERAL_PART == 0
KDECL(MODE_TICK, true)
#endif
#if GENERAL_PART == 2 || GENERAL_PART == -1
KINST(MODE_TICK, false, true)
#elif GENERAL_PART == 0
KDECL(MODE_TICK, false, true)
#endif
#if GENERAL_PART == 3 || GENERAL_PART == -1
KINST(MODE_ASSEMBLE)
KINST(MODE_FK)
#elif GENERAL_PART == 0
KDECL(MODE_ASSEMBLE)
KDECL(MODE_FK)
#endif
#if GENERAL_PART == 4 || GENERAL_PART == -1
KINST(MODE_TICK, false, false, true)
KINST(MODE_TICK, true, false, true)
#elif GENERAL_PART == 0
KDECL(MODE_TICK, false, false, true)
KDECL(MODE_TICK, true, false, true)
#endif
#if GENERAL_PART == 5 || GENERAL_PART == -1
KINST(MODE_TICK, false, true, true)
KINST(MODE_ASSEMBLE, false, false, true)
KINST(MODE_FK, false, false, true)
#elif GENERAL_PART == 0
KDECL(MODE_TICK, false, true, true)
KDECL(MODE_ASSEMBLE, false, false, true)
KDECL(MODE_FK, false, false, true)
#endif
#define TINST(...) template __global__ void wbc_tick_tp_kernel<__VA_ARGS__>(const KernelArgs, const DevModel* __restrict__, const WbcConfig* __restrict__, const DevPlan* __restrict__, const WbcTaskParams* __restrict__);
#define TDECL(...) extern template __global__ void wbc_tick_tp_kernel<__VA_ARGS__>(const KernelArgs, const DevModel* __restrict__, const WbcConfig* __restrict__, const DevPlan* __restrict__, const WbcTaskParams* __restrict__);
// the TP kernels: parts of their own (the parts above keep their code objects)
#if GENERAL_PART == 6 || GENERAL_PART == -1
TINST(MODE_TICK)
TINST(MODE_TICK, true)
TINST(MODE_ASSEMBLE)
#elif GENERAL_PART == 0
TDECL(MODE_TICK)
TDECL(MODE_TICK, true)
TDECL(MODE_ASSEMBLE)
#endif
#if GENERAL_PART == 7 || GENERAL_PART == -1
TINST(MODE_TICK, false, true)
TINST(MODE_TICK, false, true, true)
#elif GENERAL_PART == 0
TDECL(MODE_TICK, false, true)
TDECL(MODE_TICK, false, true, true)
#endif
#if GENERAL_PART == 8 || GENERAL_PART == -1
TINST(MODE_TICK, false, false, true)
TINST(MODE_TICK, true, false, true)
TINST(MODE_ASSEMBLE, false, false, true)
#elif GENERAL_PART == 0
TDECL(MODE_TICK, false, false, true)
TDECL(MODE_TICK, true, false, true)
TDECL(MODE_ASSEMBLE, false, false, true)
#endif
#undef KINST
#undef KDECL
#undef TINST
#undef TDECL
#if GENERAL_PART <= 0
// the TP kernels: the same choice of variant as launch_tick (no FK mode: it reads no weight)
static int launch_tick_tp(const KernelArgs& a, int mode, int grid, hipStream_t s, const WbcTaskParams* tp) {
  if (a.rot) {
    if (mode == MODE_TICK && (a.ws_in || a.ws_out)) hipLaunchKernelGGL((wbc_tick_tp_kernel<MODE_TICK, true, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
    else if (mode == MODE_TICK && a.presolve && a.presolve_orth == 2) hipLaunchKernelGGL((wbc_tick_tp_kernel<MODE_TICK, false, true, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
    else if (mode == MODE_TICK) hipLaunchKernelGGL((wbc_tick_tp_kernel<MODE_TICK, false, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
    else hipLaunchKernelGGL((wbc_tick_tp_kernel<MODE_ASSEMBLE, false, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
    return check_launch("tick_tp");
  }
  if (mode == MODE_TICK && (a.ws_in || a.ws_out)) hipLaunchKernelGGL((wbc_tick_tp_kernel<MODE_TICK, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
  else if (mode == MODE_TICK && a.presolve && a.presolve_orth == 2) hipLaunchKernelGGL((wbc_tick_tp_kernel<MODE_TICK, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
  else if (mode == MODE_TICK) hipLaunchKernelGGL(wbc_tick_tp_kernel<MODE_TICK>, dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
  else hipLaunchKernelGGL(wbc_tick_tp_kernel<MODE_ASSEMBLE>, dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans, tp);
  return check_launch("tick_tp");
}
int launch_tick(const KernelArgs& a, int mode, int grid, void* stream, const WbcTaskParams* tp) {
  hipStream_t s = (hipStream_t)stream;
  if (tp && mode != MODE_FK) return launch_tick_tp(a, mode, grid, s, tp);
  if (a.rot) {
    if (mode == MODE_TICK && (a.ws_in || a.ws_out)) hipLaunchKernelGGL((wbc_tick_kernel<MODE_TICK, true, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
    else if (mode == MODE_TICK && a.presolve && a.presolve_orth == 2) hipLaunchKernelGGL((wbc_tick_kernel<MODE_TICK, false, true, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
    else if (mode == MODE_TICK) hipLaunchKernelGGL((wbc_tick_kernel<MODE_TICK, false, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
    else if (mode == MODE_ASSEMBLE) hipLaunchKernelGGL((wbc_tick_kernel<MODE_ASSEMBLE, false, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
    else hipLaunchKernelGGL((wbc_tick_kernel<MODE_FK, false, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
    return check_launch("tick");
  }
  if (mode == MODE_TICK && (a.ws_in || a.ws_out)) hipLaunchKernelGGL((wbc_tick_kernel<MODE_TICK, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
  else if (mode == MODE_TICK && a.presolve && a.presolve_orth == 2) hipLaunchKernelGGL((wbc_tick_kernel<MODE_TICK, false, true>), dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
  else if (mode == MODE_TICK) hipLaunchKernelGGL(wbc_tick_kernel<MODE_TICK>, dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
  else if (mode == MODE_ASSEMBLE) hipLaunchKernelGGL(wbc_tick_kernel<MODE_ASSEMBLE>, dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
  else hipLaunchKernelGGL(wbc_tick_kernel<MODE_FK>, dim3(grid), dim3(64), 0, s, a, a.models, a.cfgs, a.plans);
  return check_launch("tick");
}
int tick_lds_bytes() { return (int)sizeof(Smem); }
#endif

}  // namespace wbc
