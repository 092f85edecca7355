// wbc_k_general.hip — the general tick kernel wbc_tick_kernel<MODE, WARM, ORTH, ROT, TP> (one instance per wavefront; tick / assemble / FK outputs).
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
// TP: per-instance weights and gains (tps [B], wbc_tick_tp / wbc_assemble_tp): row b replaces cfgs[mid]'s weight / gain block (a row that
// tp_row_bad refuses gives the instance WBC_QP_NUMERICAL). Every tick kernel takes tps; the kernels without rows get nullptr and never read it.
template <int MODE, bool WARM = false, bool ORTH = false, bool ROT = false, bool TP = false>
__global__ void __launch_bounds__(64, 2) wbc_tick_kernel(const KernelArgs A, const DevModel* __restrict__ models,
                                                         const WbcConfig* __restrict__ cfgs, const DevPlan* __restrict__ plans,
                                                         const WbcTaskParams* __restrict__ tps) {
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
  bool tp_bad = false;
  TpRow tpr = nullptr;
  if constexpr (TP) {   // (an assembly reports no status: its rows enter as they are)
    tp_bad = MODE == MODE_TICK && tp_row_bad(tps + b, lane);
    tpr = tp_bad ? (TpRow)&cfgs[mid].ee_W[0][0] : (TpRow)(tps + b);
  }
  stage_inputs(S, cur, lane, has2, has3);
  WSYNC();
  process_instance<MODE, WARM, ORTH, ROT, TP>(S, A, models[mid], cfgs[mid], plans[mid], lc, cur, b, lane, t_entry, tpr, tp_bad);
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments. With rows (TP): parts of
// their own; no FK kernel (it reads no weight).
#ifndef GENERAL_PART
#define GENERAL_PART -1      // -1: everything in one unit
#endif
#define WBC_PART GENERAL_PART
#define WBC_KERNEL wbc_tick_kernel
#define WBC_KPARAMS WBC_TICK_KPARAMS
#define GENERAL_VARIANTS(V) /* MODE, WARM, ORTH, ROT, TP */ \
  V(0, MODE_TICK, false, false, false, false)     \
  V(1, MODE_TICK, true, false, false, false)      \
  V(2, MODE_TICK, false, true, false, false)      \
  V(3, MODE_ASSEMBLE, false, false, false, false) \
  V(3, MODE_FK, false, false, false, false)       \
  V(4, MODE_TICK, false, false, true, false)      \
  V(4, MODE_TICK, true, false, true, false)       \
  V(5, MODE_TICK, false, true, true, false)       \
  V(5, MODE_ASSEMBLE, false, false, true, false)  \
  V(5, MODE_FK, false, false, true, false)        \
  V(6, MODE_TICK, false, false, false, true)      \
  V(6, MODE_TICK, true, false, false, true)       \
  V(6, MODE_ASSEMBLE, false, false, false, true)  \
  V(7, MODE_TICK, false, true, false, true)       \
  V(7, MODE_TICK, false, true, true, true)        \
  V(8, MODE_TICK, false, false, true, true)       \
  V(8, MODE_TICK, true, false, true, true)        \
  V(8, MODE_ASSEMBLE, false, false, true, true)
#if GENERAL_PART == -1
GENERAL_VARIANTS(WBC_VARIANT_INST)
#else
GENERAL_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if GENERAL_PART <= 0
static TickKernel general_variant(long long key) {
  GENERAL_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int general_variant_count() { return 0 GENERAL_VARIANTS(WBC_VARIANT_COUNT); }
int launch_tick(const KernelArgs& a, int mode, int grid, void* stream, const WbcTaskParams* tp, long long* key_out) {
  if (mode == MODE_FK) tp = nullptr;   // (FK reads no weight: no kernel with rows)
  const bool warm = mode == MODE_TICK && (a.ws_in || a.ws_out);                          // working sets and the orthonormal presolve: ticks only,
  const bool orth = mode == MODE_TICK && !warm && a.presolve && a.presolve_orth == 2;   // and a working set wins over presolve_orth == 2
  const long long key = variant_key(mode, warm, orth, a.rot != 0, tp != nullptr);
  if (key_out) *key_out = key;
  const TickKernel k = general_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3(grid), dim3(64), 0, (hipStream_t)stream, a, a.models, a.cfgs, a.plans, tp);
  return check_launch("tick");
}
int tick_lds_bytes() { return (int)sizeof(Smem); }
#endif

}  // namespace wbc
