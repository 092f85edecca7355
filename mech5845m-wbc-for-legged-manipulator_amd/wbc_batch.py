"""Batched front end of the HIP library: the many-instance form of ``RobotModel`` / ``QP``.

``WbcBatch`` owns the C handles and maps dictionaries of arrays onto the ``WbcTickIn`` / ``WbcTickOut`` /
``WbcQpData`` / ``WbcFkOut`` structs of include/wbc.h. Arrays may be numpy (host: the library stages them over
PCIe) or torch CUDA tensors (device: pointers pass straight through, nothing is copied or synchronised).
The single-instance classes in QP_Wrapper.py / Robot_Wrapper4.py are the B = 1 case of this object.
"""
import ctypes as C

import numpy as np

import wbc_capi as capi

NV, NQS = capi.V_STRIDE, capi.Q_STRIDE


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _mem_of(arrays):
    kinds = {("dev" if (_is_torch(a) and a.is_cuda) else "host") for a in arrays if a is not None}
    if len(kinds) > 1:
        raise capi.WbcError("mixing host and device arrays in one call")
    return capi.MEM_DEVICE if kinds == {"dev"} else capi.MEM_HOST


# doubles (int32 for model_id) per instance of every WbcTickIn field (include/wbc.h)
TICK_IN_WIDTH = dict(q=NQS, ee_target=15, prev_ee_target=15, trunk_target=3, prev_trunk_target=3, trunk_box_center=4,
                     ee_ref_rot=45, ee_prev_rot=45, trunk_ref_euler=3, trunk_prev_rot=9, com_target=3, com_target_vel=3,
                     model_id=1, posture_u=NV, q_con=NQS, working_set=2)
_INT32_FIELDS, _INT64_FIELDS = ("model_id", "status", "iters"), ("working_set",)


def _dtype_of(name):
    return np.int32 if name in _INT32_FIELDS else (np.int64 if name in _INT64_FIELDS else np.float64)


def _prep(a, dtype, keep, B=None, width=None, name="array", device_id=None):
    """-> pointer (the array is kept alive in `keep`). numpy arrays are made contiguous float64/int32; torch tensors are
    checked. With B / width given the array must hold exactly B x width values with B as its leading dimension: the
    kernels index raw pointers with those strides, so a wrong shape would read (or write) its neighbours' data."""
    if a is None:
        return None
    if B is not None:
        shape = tuple(a.shape)
        if len(shape) < 1 or shape[0] != B or int(np.prod(shape)) != B * width:
            raise capi.WbcError("%s: shape %s does not hold %d x %d values (leading dimension = batch)" % (name, shape, B, width))
    if _is_torch(a):
        import torch
        want = {np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dtype]
        if a.dtype != want or not a.is_contiguous():
            raise capi.WbcError("%s: device tensors must be contiguous %s" % (name, want))
        if a.is_cuda and device_id is not None and a.device.index != device_id:
            raise capi.WbcError("%s lives on cuda:%s, the handle on cuda:%d" % (name, a.device.index, device_id))
        keep.append(a)
        return a.data_ptr()
    arr = np.ascontiguousarray(a, dtype=dtype)
    keep.append(arr)
    return arr.ctypes.data


def _task_params(tp, B, keep, device_id):
    """-> pointer to the [B, 85] float64 rows (wbc_model.task_params), or None. Strict: a wrong dtype or shape is an error, never a
    silent conversion (a float32 sweep would otherwise be rounded without notice)."""
    if tp is None:
        return None
    shape = tuple(tp.shape)
    if shape != (B, capi.TASK_PARAMS_DOUBLES):
        raise capi.WbcError("task_params: shape %s, want (%d, %d)" % (shape, B, capi.TASK_PARAMS_DOUBLES))
    if _is_torch(tp):
        import torch
        if tp.dtype != torch.float64 or not tp.is_contiguous():
            raise capi.WbcError("task_params: device tensors must be contiguous torch.float64")
        if not tp.is_cuda or tp.device.index != device_id:
            raise capi.WbcError("task_params lives on %s, the handle on cuda:%d" % (tp.device, device_id))
        keep.append(tp)
        return tp.data_ptr()
    if not isinstance(tp, np.ndarray) or tp.dtype != np.float64:
        raise capi.WbcError("task_params: want a float64 numpy array or torch tensor, got %s" % getattr(tp, "dtype", type(tp)))
    arr = np.ascontiguousarray(tp)
    keep.append(arr)
    return arr.ctypes.data


class RolloutTape:
    """The tape of WbcBatch.rollout_record: `buf`, a torch uint8 tensor on the handle's device in the layout include/wbc.h states (a head of
    432 bytes per instance, then 736 bytes per instance and tick, every block strided by B), and `call`, the arguments of the recorded call."""
    _BLOCKS = (("q", np.float64, NQS), ("qdot", np.float64, NV), ("ee_target", np.float64, 15), ("prev_ee_target", np.float64, 15),
               ("trunk_target", np.float64, 3), ("prev_trunk_target", np.float64, 3), ("status", np.int32, 1), ("pad", np.int32, 1),
               ("working_set", np.int64, 2))

    def __init__(self, buf, B, ticks):
        self.buf, self.B, self.ticks, self.call = buf, int(B), int(ticks), None

    def tick(self, k):
        """-> dict of tick k's blocks as torch views into the tape: q [B,27], qdot [B,26], ee_target, prev_ee_target [B,15], trunk_target,
        prev_trunk_target [B,3], status [B] int32, working_set [B,2] int64 (blocks of inputs the call did not have hold no data; the working
        sets are recorded under option "warm_start" alone)"""
        import torch
        if not 0 <= k < self.ticks:
            raise capi.WbcError("tick %d outside [0, %d)" % (k, self.ticks))
        off = self.B * (capi.TAPE_HEAD_BYTES + k * capi.TAPE_TICK_BYTES)
        out = {}
        for name, dt, width in self._BLOCKS:
            size = self.B * width * np.dtype(dt).itemsize
            if name != "pad":
                t = self.buf[off:off + size].view({np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dt])
                out[name] = t.reshape(self.B) if width == 1 else t.reshape(self.B, width)
            off += size
        return out


class WbcBatch:
    allocator = None    # the output allocator hook (constructor argument / attribute); None: torch.empty / np.empty where the inputs live

    def __init__(self, models, max_batch, device_id=0, allocator=None):
        """allocator: a callable (like, shape, numpy dtype) -> array that replaces the default allocation of every output a wrapper
        allocates itself (everything but tick(out=...)); also settable later as the attribute `allocator` (None: the default). The
        array must be contiguous, of that shape and dtype, and live where `like` does."""
        self.lib = capi.load_library()
        if allocator is not None:
            self.allocator = allocator
        self.models = list(models) if isinstance(models, (list, tuple)) else [models]
        self.max_batch = int(max_batch)
        self._mh = []
        for m in self.models:
            h = C.c_void_p()
            capi.check(self.lib.wbc_model_create(C.byref(m.blob), C.byref(h)), self.lib)
            self._mh.append(h)
        arr = (C.c_void_p * len(self._mh))(*[h.value for h in self._mh])
        self._h = C.c_void_p()
        self.device_id = int(device_id)
        capi.check(self.lib.wbc_batch_create(arr, len(self._mh), self.max_batch, device_id, C.byref(self._h)), self.lib)
        self.cfgs = [None] * len(self.models)
        self.max_nj = max((m.njoints for m in self.models), default=0)          # FK output strides (include/wbc.h, WbcFkOut)
        self.max_nf = max((m.blob.nframes for m in self.models), default=0)

    def _stream(self, mem):
        """the handle's device's current torch stream for device buffers, the null stream for host buffers"""
        if mem == capi.MEM_DEVICE:
            import torch
            return torch.cuda.current_stream(self.device_id).cuda_stream
        return None

    def _p(self, a, dtype, keep, B=None, width=None, name="array"):
        return _prep(a, dtype, keep, B, width, name, self.device_id)

    def _batch_of(self, q, name="q"):
        if q is None or len(q.shape) != 2 or q.shape[1] != NQS:
            raise capi.WbcError("%s must be [B, %d] (padded to the largest model's nq), got %s" % (
                name, NQS, None if q is None else tuple(q.shape)))
        B = int(q.shape[0])
        if B < 1 or B > self.max_batch:
            raise capi.WbcError("B = %d outside [1, max_batch = %d]" % (B, self.max_batch))
        return B

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.wbc_batch_destroy(self._h)
            self._h = None
        for h in getattr(self, "_mh", []):
            self.lib.wbc_model_destroy(h)
        self._mh = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- settings
    def configure(self, cfg, model_index=0):
        capi.check(self.lib.wbc_batch_configure(self._h, model_index, C.byref(cfg)), self.lib)
        self.cfgs[model_index] = cfg

    def set_option(self, name, value):
        capi.check(self.lib.wbc_batch_set_option(self._h, name.encode(), int(value)), self.lib)
        self._options = dict(getattr(self, "_options", {}), **{name: int(value)})

    @property
    def task_rows(self):
        return self.lib.wbc_task_rows(self._h)

    @property
    def constraint_rows(self):
        return self.lib.wbc_constraint_rows(self._h)

    def debug_cycles(self):
        """per-phase cycle sums since the last call (profile build only; see include/wbc.h)."""
        out = (C.c_uint64 * 24)()
        capi.check(self.lib.wbc_debug_cycles(self._h, out), self.lib)
        return [int(v) for v in out]

    def synchronize(self, stream=None):
        capi.check(self.lib.wbc_batch_synchronize(self._h, stream), self.lib)

    def stat(self, name, stream=None):
        """wbc_batch_get_stat: "last_path" (0 general, 1 compact sim3, 2 packed sim3, 3 packed orth — equality-only or INEQ variant —, 4 packed box), "last_orth", "last_posture_par",
        "last_update_packed", "last_qp_path" (problems per wavefront of the last stand-alone QP call: 1, 2 or 4), "last_tick_variant" /
        "last_qp_variant" (the variant-table row of the last tick / assemble / fk and stand-alone QP launch: wbc_capi.variant_args), "last_grad_variant" / "last_gradq_variant" / "last_stepvjp_variant" / "last_rollvjp_variant" / "last_trackvjp_variant" (the same for the last wbc_tick_vjp / wbc_tick_vjp_state / wbc_step_vjp launch, the last link-kernel launch of wbc_rollout_vjp and the last track-adjoint launch of wbc_rollout_vjp_tracks), "last_tick_fixd" (1: the last tick ran the
        packed sim3 kernel's FIXD form, option "sim3p_fixd"), "deferred_last", "pivoted_last", "wave_order_slices", "sim3_lds_bytes", "tick_lds_bytes", "orthp_lds_bytes"."""
        v = C.c_int64()
        capi.check(self.lib.wbc_batch_get_stat(self._h, name.encode(), stream, C.byref(v)), self.lib)
        return int(v.value)

    # ---- helpers
    def _tick_in(self, inputs, keep, B):
        unknown = set(inputs) - set(TICK_IN_WIDTH)
        if unknown:
            raise capi.WbcError("unknown tick inputs %s" % sorted(unknown))
        t = capi.WbcTickIn()
        for name, _ in capi.WbcTickIn._fields_:
            a = inputs.get(name)
            if a is not None:
                setattr(t, name, self._p(a, _dtype_of(name), keep, B, TICK_IN_WIDTH[name], name))
        return t

    def _outs(self, out, widths, keep, B, struct):
        for k, v in out.items():
            if k not in widths:
                raise capi.WbcError("unknown output %r" % k)
            setattr(struct, k, self._p(v, _dtype_of(k), keep, B, widths[k], k))
        return struct

    # which input of the configuration a gradient output belongs to (the library's OutRow tables; an output not named here is always offered)
    _NEEDS = dict(d_ee_target="ee", d_prev_ee_target="ee", d_trunk_target="trunk", d_prev_trunk_target="trunk", d_trunk_target_step="trunk",
                  d_com_target="com", d_com_target_vel="com", d_posture_u="posture_u", d_trunk_box_center="con_trunk")
    _ROLLOUT_NEEDS = dict(_NEEDS, d_ee_target="ee_est", d_ee_target_step="ee_est")     # the estimator of RUNNING mode reads ee_target too

    def _offered(self, fields, needs=_NEEDS, mode=None):
        """the names of `fields` whose input the handle's configuration reads (mode: the roll-out's; RUNNING has the estimator)"""
        c = self.cfgs[0]
        ee = any(c.task_ee[e] for e in range(capi.NEE))
        reads = dict(ee=ee, ee_est=ee or mode == capi.ROLLOUT_RUNNING, trunk=c.task_trunk, com=c.task_com, con_trunk=c.con_trunk,
                     posture_u=all(cf is not None and cf.task_joint >= capi.JOINT_MANI for cf in self.cfgs))
        return tuple(k for k in fields if k not in needs or reads[needs[k]])

    def _grad_outs(self, fields, struct, like, B, keep, want, default, out, extras=("grad_status",)):
        """-> (out, o): the outputs of a *_vjp method and the struct that points at them. fields: name -> per-instance shape. out None: the
        arrays of `want` (None: default()) are allocated where `like` lives, and the int32 [B] `extras`; else the caller's arrays by name."""
        if out is None:
            names = default() if want is None else tuple(want)
            unknown = set(names) - set(fields)
            if unknown:
                raise capi.WbcError("unknown gradients %s (known: %s)" % (sorted(unknown), ", ".join(fields)))
            out = {k: self._alloc(like, (B,) + fields[k]) for k in names}
            out.update({k: self._alloc(like, (B,), np.int32) for k in extras})
        o = struct()
        for k, a in out.items():
            if k in extras:
                setattr(o, k, self._p(a, np.int32, keep, B, 1, k))
            elif k in fields:
                setattr(o, k, self._p(a, np.float64, keep, B, int(np.prod(fields[k])), k))
            else:
                raise capi.WbcError("unknown output %r" % k)
        return out, o

    def _alloc(self, like, shape, dtype=np.float64):
        if self.allocator is not None:
            return self.allocator(like, shape, dtype)
        if like is not None and _is_torch(like):
            import torch
            return torch.empty(shape, dtype={np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dtype], device=like.device)
        return np.empty(shape, dtype=dtype)

    # ---- entry points
    def fk(self, q, model_id=None, want=("oMi", "oMf", "J", "com", "Jcom")):
        """updateState's kinematics: returns dict(oMi [B,nj,12], oMf [B,nf,12], J [B,6,26], com [B,3], Jcom [B,3,26]);
        nj / nf are the LARGEST model's joint / frame counts (rows beyond an instance's own model are zero)."""
        keep = []
        mem = _mem_of([q, model_id])
        B = self._batch_of(q)
        nj, nf = self.max_nj, self.max_nf
        shapes = dict(oMi=(B, nj, 12), oMf=(B, nf, 12), J=(B, 6, NV), com=(B, 3), Jcom=(B, 3, NV))
        out = {k: self._alloc(q, shapes[k]) for k in want}
        o = capi.WbcFkOut()
        for k, v in out.items():
            setattr(o, k, self._p(v, np.float64, keep))
        capi.check(self.lib.wbc_fk_jacobians(self._h, B, self._p(q, np.float64, keep), self._p(model_id, np.int32, keep, B, 1, "model_id"),
                                              mem, C.byref(o), self._stream(mem)), self.lib)
        return out

    def assemble(self, inputs, dt, want=("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub"), task_params=None):
        """qpA/qpb/findConstraints/velDamperJointConstraints + H, g for every instance. task_params: [B, 85] per-instance weights and
        gains (wbc_model.task_params; wbc_assemble_tp), None = the configuration's."""
        keep = []
        mem = _mem_of(list(inputs.values()) + [task_params])
        q = inputs.get("q")
        B = self._batch_of(q)
        m, p = self.task_rows, self.constraint_rows
        shapes = dict(A=(B, m, NV), b=(B, m), H=(B, NV, NV), g=(B, NV), C=(B, p, NV), Clb=(B, p), Cub=(B, p), lb=(B, NV), ub=(B, NV))
        out = {k: self._alloc(q, shapes[k]) for k in want}
        o = capi.WbcQpData()
        for k, v in out.items():
            setattr(o, k, self._p(v, np.float64, keep))
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        capi.check(self.lib.wbc_assemble_tp(self._h, B, C.byref(tin), tp, float(dt), mem, C.byref(o), self._stream(mem)), self.lib)
        return out

    _TICK_OUT_WIDTH = dict(qdot=NV, status=1, iters=1, q_next=NQS, working_set=2)

    def tick(self, inputs, dt, want_q_next=False, out=None, want_working_set=False, task_params=None):
        """One runWBC tick per instance up to the QP (+ integrate): returns dict(qdot, status, iters[, q_next][, working_set]).
        inputs["working_set"] (int64 [B,2], the previous tick's out["working_set"]) warm-starts the QP (include/wbc.h).
        task_params: [B, 85] per-instance weights and gains (wbc_model.task_params; wbc_tick_tp), None = the configuration's."""
        keep = []
        q = inputs.get("q")
        B = self._batch_of(q)
        if out is None:
            out = dict(qdot=self._alloc(q, (B, NV)), status=self._alloc(q, (B,), np.int32), iters=self._alloc(q, (B,), np.int32))
            if want_q_next:
                out["q_next"] = self._alloc(q, (B, NQS))
            if want_working_set:
                out["working_set"] = self._alloc(q, (B, 2), np.int64)
        mem = _mem_of(list(inputs.values()) + list(out.values()) + [task_params])
        o = self._outs(out, self._TICK_OUT_WIDTH, keep, B, capi.WbcTickOut())
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        capi.check(self.lib.wbc_tick_tp(self._h, B, C.byref(tin), tp, float(dt), mem, C.byref(o), self._stream(mem)), self.lib)
        return out

    def make_tick_call(self, inputs, out, dt, task_params=None):
        """Bind device tensors once; the returned closure issues exactly one wbc_tick (wbc_tick_tp with task_params, [B, 85] on the
        device: read afresh by every call) on the handle's current stream."""
        keep = []
        if _mem_of(list(inputs.values()) + list(out.values()) + [task_params]) != capi.MEM_DEVICE:
            raise capi.WbcError("make_tick_call wants device tensors")
        B = self._batch_of(inputs.get("q"))
        o = self._outs(out, self._TICK_OUT_WIDTH, keep, B, capi.WbcTickOut())
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        lib, h, dtv, dev = self.lib, self._h, float(dt), self.device_id
        import torch

        def call():
            rc = lib.wbc_tick_tp(h, B, C.byref(tin), tp, dtv, capi.MEM_DEVICE, C.byref(o), torch.cuda.current_stream(dev).cuda_stream)
            if rc:
                capi.check(rc, lib)
        call._keep = keep
        return call

    def qp_solve(self, H, g, C_=None, lb=None, ub=None, Clb=None, Cub=None, working_set=None, want_working_set=False):
        """Batched QP.solveQP given H, g. H [B,n,n], C_ [B,p,n] (row-major rows), returns (x, status, iters).
        working_set [B,2] int64 (include/wbc.h wbc_qp_solve) hot-starts the solve; want_working_set appends the final one to the result."""
        keep = []
        mem = _mem_of([H, g, C_, lb, ub, Clb, Cub, working_set])
        if len(H.shape) != 3 or H.shape[1] != H.shape[2]:
            raise capi.WbcError("H must be [B, n, n], got %s" % (tuple(H.shape),))
        B, n = H.shape[0], H.shape[-1]
        if C_ is not None and (len(C_.shape) != 3 or C_.shape[2] != n):
            raise capi.WbcError("C must be [B, p, %d], got %s" % (n, tuple(C_.shape)))
        p = 0 if C_ is None else C_.shape[-2]
        x, st, it = self._alloc(H, (B, n)), self._alloc(H, (B,), np.int32), self._alloc(H, (B,), np.int32)
        wso = self._alloc(H, (B, 2), np.int64) if want_working_set else None
        f = np.float64
        P = self._p
        capi.check(self.lib.wbc_qp_solve(self._h, B, n, p, P(H, f, keep), P(g, f, keep, B, n, "g"), P(C_, f, keep, B, p * n, "C"),
                                          P(lb, f, keep, B, n, "lb"), P(ub, f, keep, B, n, "ub"), P(Clb, f, keep, B, p, "Clb"),
                                          P(Cub, f, keep, B, p, "Cub"), mem,
                                          P(x, f, keep), P(st, np.int32, keep), P(it, np.int32, keep),
                                          P(working_set, np.int64, keep, B, 2, "working_set"), P(wso, np.int64, keep), self._stream(mem)), self.lib)
        return (x, st, it, wso) if want_working_set else (x, st, it)

    def qp_solve_ls(self, A, b, C_=None, lb=None, ub=None, Clb=None, Cub=None, use_mfma=None, want_Hg=False, working_set=None,
                    want_working_set=False):
        """Batched QP(A, b, ...).solveQP(): H = A'A and g = -A'b are formed on the device (QP_Wrapper.py:17-18);
        use_mfma: True / False, None = matrix cores from WBC_MFMA_AUTO_ROWS rows of A on. working_set / want_working_set: as in
        qp_solve (solveQPHotstart); the final set comes last in the returned tuple."""
        keep = []
        mem = _mem_of([A, b, C_, lb, ub, Clb, Cub, working_set])
        if len(A.shape) != 3:
            raise capi.WbcError("A must be [B, m, n], got %s" % (tuple(A.shape),))
        B, m, n = A.shape
        if C_ is not None and (len(C_.shape) != 3 or C_.shape[2] != n):
            raise capi.WbcError("C must be [B, p, %d], got %s" % (n, tuple(C_.shape)))
        p = 0 if C_ is None else C_.shape[-2]
        x, st, it = self._alloc(A, (B, n)), self._alloc(A, (B,), np.int32), self._alloc(A, (B,), np.int32)
        Ho = self._alloc(A, (B, n, n)) if want_Hg else None
        go = self._alloc(A, (B, n)) if want_Hg else None
        wso = self._alloc(A, (B, 2), np.int64) if want_working_set else None
        f = np.float64
        P = self._p
        capi.check(self.lib.wbc_qp_solve_ls(self._h, B, m, n, p, P(A, f, keep), P(b, f, keep, B, m, "b"), P(C_, f, keep, B, p * n, "C"),
                                             P(lb, f, keep, B, n, "lb"), P(ub, f, keep, B, n, "ub"), P(Clb, f, keep, B, p, "Clb"),
                                             P(Cub, f, keep, B, p, "Cub"), mem,
                                             -1 if use_mfma is None else int(bool(use_mfma)), P(x, f, keep), P(st, np.int32, keep), P(it, np.int32, keep),
                                             P(Ho, f, keep), P(go, f, keep),
                                             P(working_set, np.int64, keep, B, 2, "working_set"), P(wso, np.int64, keep), self._stream(mem)), self.lib)
        out = (x, st, it, Ho, go) if want_Hg else (x, st, it)
        return out + (wso,) if want_working_set else out

    def qp_certificate(self, x, H=None, g=None, A=None, b=None, C_=None, lb=None, ub=None, Clb=None, Cub=None, status=None, working_set=None,
                       v=None):
        """wbc_qp_certificate (include/wbc.h): dual solution, KKT certificate and — with v [B,n] = dL/dx — the sensitivities of solved QPs, one
        kernel launch. Give H [B,n,n], g or A [B,m,n], b. status / working_set: what the solve returned (int32 [B] / int64 [B,2]; optional).
        Returns dict(y_bounds [B,n], y_rows [B,p], kkt [B,4], objective [B], n_active [B], cert_status [B][, sens_x, sens_bounds, sens_rows])."""
        keep = []
        mem = _mem_of([x, H, g, A, b, C_, lb, ub, Clb, Cub, status, working_set, v])
        if x is None or len(x.shape) != 2:
            raise capi.WbcError("x must be [B, n], got %s" % (None if x is None else tuple(x.shape),))
        B, n = int(x.shape[0]), int(x.shape[1])
        if C_ is not None and (len(C_.shape) != 3 or C_.shape[2] != n):
            raise capi.WbcError("C must be [B, p, %d], got %s" % (n, tuple(C_.shape)))
        p = 0 if C_ is None else int(C_.shape[1])
        if A is not None and (len(A.shape) != 3 or A.shape[2] != n):
            raise capi.WbcError("A must be [B, m, %d], got %s" % (n, tuple(A.shape)))
        m = 0 if A is None else int(A.shape[1])
        f, P = np.float64, self._p
        q = capi.WbcQpProblem()
        q.n, q.p, q.m = n, p, m
        q.H, q.g = P(H, f, keep, B, n * n, "H"), P(g, f, keep, B, n, "g")
        q.A, q.b = P(A, f, keep, B, m * n, "A"), P(b, f, keep, B, m, "b")
        q.C, q.lb, q.ub = P(C_, f, keep, B, p * n, "C"), P(lb, f, keep, B, n, "lb"), P(ub, f, keep, B, n, "ub")
        q.Clb, q.Cub = P(Clb, f, keep, B, p, "Clb"), P(Cub, f, keep, B, p, "Cub")
        q.x, q.v = P(x, f, keep, B, n, "x"), P(v, f, keep, B, n, "v")
        q.status, q.working_set = P(status, np.int32, keep, B, 1, "status"), P(working_set, np.int64, keep, B, 2, "working_set")
        shapes = dict(y_bounds=((B, n), f), y_rows=((B, p), f), kkt=((B, 4), f), objective=((B,), f), n_active=((B,), np.int32),
                      cert_status=((B,), np.int32))
        if v is not None:
            shapes.update(sens_x=((B, n), f), sens_bounds=((B, n), f), sens_rows=((B, p), f))
        out = {k: self._alloc(x, s, d) for k, (s, d) in shapes.items()}
        o = capi.WbcQpCert()
        for k, a in out.items():
            if a.shape[-1] != 0 or len(a.shape) == 1:          # (p == 0: the row outputs are empty and stay NULL)
                setattr(o, k, P(a, shapes[k][1], keep))
        capi.check(self.lib.wbc_qp_certificate(self._h, B, C.byref(q), C.byref(o), mem, self._stream(mem)), self.lib)
        return out

    def _padding_rows(self, model_id, B, like):
        """[B, k, 26] rows e_c, one per column c >= nv of the instance's own model (k = 26 - the smallest nv of the handle; zero rows where an
        instance's model has fewer padded columns), or None when every model fills the 26 columns. wbc_assemble leaves the padded columns of A
        zero (H_dd = 1 and bounds 0 in H's form: include/wbc.h), so A'A alone is singular there; with these rows the (A, b) form is the tick's
        problem for every model."""
        nvs = [m.nv for m in self.models]
        k = NV - min(nvs)
        if k <= 0:
            return None
        if _is_torch(like):
            import torch
            nv = torch.tensor(nvs, dtype=torch.int64, device=like.device)
            nv_b = nv[model_id.to(torch.int64).clamp(0, len(nvs) - 1)] if model_id is not None else nv[:1].expand(B)
            col = nv_b[:, None] + torch.arange(k, device=like.device)[None, :]
            return (torch.arange(NV, device=like.device)[None, None, :] == col[:, :, None]).to(torch.float64).contiguous()
        nv = np.asarray(nvs, dtype=np.int64)
        nv_b = nv[np.clip(np.asarray(model_id, dtype=np.int64), 0, len(nvs) - 1)] if model_id is not None else np.full(B, nv[0])
        col = nv_b[:, None] + np.arange(k)[None, :]
        return (np.arange(NV)[None, None, :] == col[:, :, None]).astype(np.float64)

    def tick_certificate(self, inputs, dt, task_params=None, v=None, tick=None):
        """One tick with its certificate, all on the device: wbc_assemble[_tp] (A, b, C, bounds), wbc_tick[_tp] with the working set out, then
        wbc_qp_certificate in the (A, b) form on the full problem (the tick's working set is in the full problem's indexing on every path).
        v [B,26]: dL/dqdot for the sensitivities. tick: a tick of these inputs already run with the working set out (dict(qdot, status,
        working_set)); None runs it. A model with fewer than 26 velocity columns gets unit rows on its padded columns (_padding_rows).
        Returns dict(qdot, status, iters, working_set) plus qp_certificate's entries."""
        d = self.assemble(inputs, dt, want=("A", "b", "C", "Clb", "Cub", "lb", "ub"), task_params=task_params)
        t = self.tick(inputs, dt, want_working_set=True, task_params=task_params) if tick is None else tick
        has_rows = d["C"].shape[1] > 0
        A, b = d["A"], d["b"]
        pad = self._padding_rows(inputs.get("model_id"), A.shape[0], A)
        if pad is not None:
            if _is_torch(A):
                import torch
                A, b = torch.cat([A, pad], dim=1).contiguous(), torch.cat([b, torch.zeros_like(pad[:, :, 0])], dim=1).contiguous()
            else:
                A, b = np.concatenate([A, pad], axis=1), np.concatenate([b, np.zeros(pad.shape[:2])], axis=1)
        # lb / ub as wbc_assemble returns them: +-1e30 (no bound) for an instance whose model's configuration has the velocity box off
        c = self.qp_certificate(t["qdot"], A=A, b=b, C_=d["C"] if has_rows else None, lb=d["lb"], ub=d["ub"],
                                Clb=d["Clb"] if has_rows else None, Cub=d["Cub"] if has_rows else None,
                                status=t["status"], working_set=t["working_set"], v=v)
        return dict(t, **c)

    def default_grad_wants(self):
        """the gradients wbc_tick_vjp offers under the handle's configuration (names of capi.TICK_GRAD_FIELDS)"""
        return self._offered(capi.TICK_GRAD_FIELDS)

    def tick_vjp(self, inputs, dt, qdot, sens_x, status=None, cert_status=None, task_params=None, want=None, out=None):
        """wbc_tick_vjp (include/wbc.h): dL/d(task weights, gains, targets) of solved ticks from x = qdot [B,26] and the certificate's
        u = sens_x [B,26], one kernel launch. want: names of capi.TICK_GRAD_FIELDS (None: default_grad_wants()); out: caller's arrays by
        those names (and "grad_status") instead. Returns dict(<want>..., grad_status [B] int32)."""
        keep = []
        B = self._batch_of(inputs.get("q"))
        out, o = self._grad_outs(capi.TICK_GRAD_FIELDS, capi.WbcTickGrad, qdot, B, keep, want, self.default_grad_wants, out)
        mem = _mem_of(list(inputs.values()) + list(out.values()) + [task_params, qdot, sens_x, status, cert_status])
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        f, P = np.float64, self._p
        capi.check(self.lib.wbc_tick_vjp(self._h, B, C.byref(tin), tp, float(dt), P(qdot, f, keep, B, NV, "qdot"), P(sens_x, f, keep, B, NV, "sens_x"),
                                         P(status, np.int32, keep, B, 1, "status"), P(cert_status, np.int32, keep, B, 1, "cert_status"), mem,
                                         C.byref(o), self._stream(mem)), self.lib)
        return out

    def tick_grad(self, inputs, dt, v, task_params=None, want=None):
        """The tick as a layer: tick_certificate(..., v=v) and then wbc_tick_vjp on its qdot and sens_x, on the device throughout when the
        inputs are. v [B,26] = dL/dqdot. Returns the tick's and the certificate's entries plus the gradients (tick_vjp's names) and grad_status."""
        c = self.tick_certificate(inputs, dt, task_params=task_params, v=v)
        g = self.tick_vjp(inputs, dt, c["qdot"], c["sens_x"], status=c["status"], cert_status=c["cert_status"], task_params=task_params, want=want)
        return dict(c, **g)

    def tick_vjp_state(self, inputs, dt, qdot, sens_x, sens_bounds=None, sens_rows=None, y_rows=None, status=None, cert_status=None,
                       working_set=None, task_params=None, want=None, out=None):
        """wbc_tick_vjp_state (include/wbc.h): dL/dq in tangent coordinates (d_q [B,26]: q (+) delta = pin.integrate(q, delta)) and
        dL/d trunk_box_center [B,4] of solved ticks from x = qdot and the certificate's u = sens_x, w = sens_bounds / sens_rows, y = y_rows, one
        kernel launch. want: names of capi.TICK_STATE_GRAD_FIELDS (None: d_q, and d_trunk_box_center with the trunk constraint); out: caller's
        arrays by those names (and "grad_status") instead. posture_u and the orientation references are held constant; q_con is refused.
        Returns dict(<want>..., grad_status [B] int32)."""
        keep = []
        B = self._batch_of(inputs.get("q"))
        out, o = self._grad_outs(capi.TICK_STATE_GRAD_FIELDS, capi.WbcTickStateGrad, qdot, B, keep, want,
                                 lambda: self._offered(capi.TICK_STATE_GRAD_FIELDS), out)
        mem = _mem_of(list(inputs.values()) + list(out.values()) + [task_params, qdot, sens_x, sens_bounds, sens_rows, y_rows, status, cert_status,
                                                                    working_set])
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        f, P, p = np.float64, self._p, self.constraint_rows
        sn = capi.WbcTickSens()
        sn.qdot, sn.sens_x, sn.sens_bounds = P(qdot, f, keep, B, NV, "qdot"), P(sens_x, f, keep, B, NV, "sens_x"), P(sens_bounds, f, keep, B, NV, "sens_bounds")
        if p > 0:
            sn.sens_rows, sn.y_rows = P(sens_rows, f, keep, B, p, "sens_rows"), P(y_rows, f, keep, B, p, "y_rows")
        sn.status, sn.cert_status = P(status, np.int32, keep, B, 1, "status"), P(cert_status, np.int32, keep, B, 1, "cert_status")
        sn.working_set = P(working_set, np.int64, keep, B, 2, "working_set")
        capi.check(self.lib.wbc_tick_vjp_state(self._h, B, C.byref(tin), tp, float(dt), C.byref(sn), mem, C.byref(o), self._stream(mem)), self.lib)
        return out

    def tick_grad_q(self, inputs, dt, v, task_params=None, want=None):
        """The tick as a layer over its state: tick_certificate(..., v=v) and then wbc_tick_vjp_state on its qdot, sensitivities, duals and working
        set, on the device throughout when the inputs are. v [B,26] = dL/dqdot. Returns the tick's and the certificate's entries plus d_q [B,26]
        (tangent coordinates; wbc_workload.tangent_to_raw for raw ones), d_trunk_box_center [B,4] with the trunk constraint, and grad_status."""
        c = self.tick_certificate(inputs, dt, task_params=task_params, v=v)
        g = self.tick_vjp_state(inputs, dt, c["qdot"], c["sens_x"], sens_bounds=c["sens_bounds"], sens_rows=c["sens_rows"], y_rows=c["y_rows"],
                                status=c["status"], cert_status=c["cert_status"], working_set=c["working_set"], task_params=task_params, want=want)
        return dict(c, **g)

    def posture_target(self, q, model_id=None, want_q_after=True):
        """qpJointb's "MANI" / "HYBRID" posture target u [B,26] under the configured mode (Robot_Wrapper4.py:1220-1260),
        and the configuration the reference's state is left at, q_after [B,27]."""
        keep = []
        mem = _mem_of([q, model_id])
        B = self._batch_of(q)
        u = self._alloc(q, (B, NV))
        qa = self._alloc(q, (B, NQS)) if want_q_after else None
        f = np.float64
        capi.check(self.lib.wbc_posture_target(self._h, B, self._p(q, f, keep), self._p(model_id, np.int32, keep, B, 1, "model_id"), mem,
                                                self._p(u, f, keep), self._p(qa, f, keep), self._stream(mem)), self.lib)
        return (u, qa) if want_q_after else u

    def update_state(self, q_cur, q_next, foot_targets, imu=None, model_id=None):
        """The tail of runWBC (Robot_Wrapper4.py:1397-1399): updateState(joint_config, base_config, running=True) with the
        foot-anchored base estimator trunkWorldPos (:1297-1327). Returns the new current_joint_config [B,27]."""
        keep = []
        mem = _mem_of([q_cur, q_next, foot_targets, imu, model_id])
        B = self._batch_of(q_cur, "q_cur")
        qn = self._alloc(q_cur, (B, NQS))
        f = np.float64
        P = self._p
        capi.check(self.lib.wbc_update_state(self._h, B, P(q_cur, f, keep), P(q_next, f, keep, B, NQS, "q_next"), P(imu, f, keep, B, 4, "imu"),
                                              P(foot_targets, f, keep, B, 15, "foot_targets"), P(model_id, np.int32, keep, B, 1, "model_id"), mem,
                                              P(qn, f, keep), self._stream(mem)), self.lib)
        return qn

    def step_vjp(self, q_cur, qdot, foot_targets, g, dt, imu=None, model_id=None, mode=capi.ROLLOUT_RUNNING, want=None, out=None):
        """wbc_step_vjp (include/wbc.h): the state step between two ticks as a layer. For q_new = update_state(q_cur, integrate(q_cur, qdot, dt),
        foot_targets, imu) (mode ROLLOUT_WARMUP: q_new = integrate(q_cur, qdot, dt)) and g [B,26] = dL/d delta_new in the tangent coordinates at
        q_new: d_q [B,26] (tangent coordinates at q_cur; wbc_workload.tangent_to_raw for raw ones), d_qdot [B,26], d_foot_targets [B,5,3], one
        kernel launch. want: names of capi.STEP_GRAD_FIELDS (None: all three); out: caller's arrays by those names (and "grad_status") instead.
        The IMU quaternion is held constant. Returns dict(<want>..., grad_status [B] int32)."""
        keep = []
        B = self._batch_of(q_cur, "q_cur")
        out, o = self._grad_outs(capi.STEP_GRAD_FIELDS, capi.WbcStepGrad, q_cur, B, keep, want, lambda: tuple(capi.STEP_GRAD_FIELDS), out)
        mem = _mem_of([q_cur, qdot, foot_targets, g, imu, model_id] + list(out.values()))
        f, P = np.float64, self._p
        capi.check(self.lib.wbc_step_vjp(self._h, B, P(q_cur, f, keep), P(qdot, f, keep, B, NV, "qdot"), P(foot_targets, f, keep, B, 15, "foot_targets"),
                                          P(imu, f, keep, B, 4, "imu"), P(model_id, np.int32, keep, B, 1, "model_id"), float(dt), int(mode),
                                          P(g, f, keep, B, NV, "g"), mem, C.byref(o), self._stream(mem)), self.lib)
        return out

    # ---- roll-outs: every entry point builds its outputs and its WbcRollout with _rollout_base and adds the structs of its own
    def _rollout_base(self, inputs, B, keep, ticks, mode, hold_ticks=0, ee_target_step=None, trunk_target_step=None, imu=None, want_trace=False):
        """-> (out, r): the outputs every roll-out returns (q, qdot, ee_target, status, iters[, grip_trace [ticks + hold_ticks, B, 3]]) and the
        WbcRollout that points at them and at the step / imu inputs"""
        q = inputs["q"]
        K, H = int(ticks), int(hold_ticks)
        out = dict(q=self._alloc(q, (B, NQS)), qdot=self._alloc(q, (B, NV)), ee_target=self._alloc(q, (B, 5, 3)),
                   status=self._alloc(q, (B,), np.int32), iters=self._alloc(q, (B,), np.int32))
        if want_trace:
            out["grip_trace"] = self._alloc(q, (K + H, B, 3))
        r = capi.WbcRollout()
        r.ticks, r.mode, r.hold_ticks = K, int(mode), H
        f = np.float64
        P = self._p
        r.ee_target_step, r.trunk_target_step, r.imu = (P(ee_target_step, f, keep, B, 15, "ee_target_step"),
                                                        P(trunk_target_step, f, keep, B, 3, "trunk_target_step"), P(imu, f, keep, B, 4, "imu"))
        r.q_final, r.qdot_last, r.ee_target_final = P(out["q"], f, keep), P(out["qdot"], f, keep), P(out["ee_target"], f, keep)
        r.status_max, r.iters_sum = P(out["status"], np.int32, keep), P(out["iters"], np.int32, keep)
        if want_trace:
            r.grip_trace = P(out["grip_trace"], f, keep)
        return out, r

    @staticmethod
    def _check_ticks_groups(B, ticks, group_size):
        """the checks the scored roll-outs share -> group_size as an int"""
        M = int(group_size)
        if M < 0 or (M > 0 and B % M != 0):
            raise capi.WbcError("group_size = %d does not divide B = %d" % (M, B))
        if int(ticks) < 1:
            raise capi.WbcError("ticks = %d, want >= 1" % ticks)
        return M

    def rollout(self, inputs, dt, ticks, ee_target_step=None, trunk_target_step=None, imu=None, want_trace=True,
                mode=capi.ROLLOUT_RUNNING, hold_ticks=0, task_params=None):
        """K closed-loop ticks on the device: tick -> update_state -> reference-state side effects ->
        targets advance by their step; then `hold_ticks` more ticks with the targets held. mode: ROLLOUT_RUNNING
        (updateState(running=True): IMU fed back, base re-estimated from the stance feet) or ROLLOUT_WARMUP
        (updateState(running=False), the loop of setInitialState). Returns dict(q, qdot, ee_target, status, iters[,
        grip_trace [K + hold, B, 3]]). task_params: [B, 85] per-instance weights and gains for every tick (wbc_rollout_tp)."""
        keep = []
        mem = _mem_of(list(inputs.values()) + [ee_target_step, trunk_target_step, imu, task_params])
        B = self._batch_of(inputs.get("q"))
        out, r = self._rollout_base(inputs, B, keep, ticks, mode, hold_ticks, ee_target_step, trunk_target_step, imu, want_trace)   # (ticks and hold_ticks: the library's own check)
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        capi.check(self.lib.wbc_rollout_tp(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), mem, self._stream(mem)), self.lib)
        return out

    def rollout_record(self, inputs, dt, ticks, ee_target_step=None, trunk_target_step=None, imu=None, mode=capi.ROLLOUT_RUNNING,
                       task_params=None, want_trace=True, tape=None, tracks=None, score=(), group_size=0, watch=(), watch_group_size=0,
                       watch_trace=False):
        """wbc_rollout_record (include/wbc.h): rollout(..., want_trace=False) that also writes a tape for rollout_vjp. Returns (out, tape): out
        is rollout's dict plus q_trace [K, B, 27] (the state after every tick; want_trace); tape is a RolloutTape — device memory of
        wbc_rollout_tape_bytes(B, K) bytes (a torch uint8 tensor on the handle's device, allocated here or the caller's `tape.buf` when a
        RolloutTape of the same B and K is passed back in) together with the call's arguments, which rollout_vjp needs again. The ticks run
        exactly as rollout's do: under option "warm_start" they return working sets and the tape holds them. No hold ticks;
        inputs must not hold q_con; posture modes MANI / HYBRID need inputs["posture_u"].
        tracks (rollout_tracks' list of dicts; None: the call above, argument for argument): wbc_rollout_record_tracks — rollout_tracks(...,
        score, group_size) that also writes the tape; out then holds rollout_tracks' results too, and rollout_vjp returns the gradients
        with respect to every track's points, tangents and du. Not together with ee_target_step.
        watch (rollout_watch's families; empty: the calls above): wbc_rollout_record_watch — rollout_watch(..., watch, group_size =
        watch_group_size, want_trace = watch_trace) that also writes the tape, with or without tracks; out then holds rollout_watch's
        results too (slack_min, slack_final, slack_min_tick, ... [n_w, B], slack_trace [K, n_w, B]), whose cotangents rollout_vjp takes as
        watch_seed."""
        import torch
        fams = sorted({self._slack_family(f_) for f_ in watch})
        if len(fams) != len(list(watch)):
            raise capi.WbcError("watch: a family is listed twice")
        keep = []
        arrays = []
        if tracks is not None:
            tracks = list(tracks)
            if not 1 <= len(tracks) <= capi.MAX_TRACKS:
                raise capi.WbcError("tracks: %d given, want 1..%d" % (len(tracks), capi.MAX_TRACKS))
            arrays = self._track_arrays(tracks)
        elif len(list(score)):
            raise capi.WbcError("score: needs tracks")
        mem = _mem_of(list(inputs.values()) + arrays + [ee_target_step, trunk_target_step, imu, task_params])
        B = self._batch_of(inputs.get("q"))
        K = int(ticks)
        out, r = self._rollout_base(inputs, B, keep, K, mode, 0, ee_target_step, trunk_target_step, imu, False)
        tk = sc = None
        if tracks is not None:
            M = self._check_ticks_groups(B, K, group_size)
            tk, _ = self._tracks_struct(tracks, B, keep)
            frames = sorted({self._target_index(s_, "score") for s_ in score})
            if len(frames) != len(list(score)):
                raise capi.WbcError("score: a frame is listed twice")
            if inputs.get("trunk_target") is not None:
                out["trunk_target"] = self._alloc(inputs["q"], (B, 3))
                tk.trunk_target_final = self._p(out["trunk_target"], np.float64, keep)
            sc = self._scores_struct(out, inputs["q"], frames, B, K, M, False, keep)
        if want_trace and K >= 1:
            out["q_trace"] = self._alloc(inputs["q"], (K, B, NQS))
        nbytes = int(self.lib.wbc_rollout_tape_bytes(B, K))
        if tape is None or tape.B != B or tape.ticks != K:
            tape = RolloutTape(torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:%d" % self.device_id), B, K)
        tape.call = dict(inputs=dict(inputs), dt=float(dt), imu=imu, mode=int(mode), task_params=task_params,
                         warm_start=getattr(self, "_options", {}).get("warm_start", 0),
                         tracks=None if tracks is None else [dict(t) for t in tracks])
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        if fams:
            wt = self._watch_struct(out, inputs["q"], fams, B, K, self._check_ticks_groups(B, K, watch_group_size), watch_trace, keep)
            capi.check(self.lib.wbc_rollout_record_watch(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), C.byref(tk) if tk is not None else None,
                                                         C.byref(sc) if sc is not None else None, C.byref(wt), tape.buf.data_ptr(), nbytes,
                                                         self._p(out.get("q_trace"), np.float64, keep), mem, self._stream(mem)), self.lib)
            return out, tape
        if tk is not None:
            capi.check(self.lib.wbc_rollout_record_tracks(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), C.byref(tk),
                                                          C.byref(sc) if sc is not None else None, tape.buf.data_ptr(), nbytes,
                                                          self._p(out.get("q_trace"), np.float64, keep), mem, self._stream(mem)), self.lib)
            return out, tape
        capi.check(self.lib.wbc_rollout_record(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), tape.buf.data_ptr(), nbytes,
                                                self._p(out.get("q_trace"), np.float64, keep), mem, self._stream(mem)), self.lib)
        return out, tape

    def rollout_vjp(self, tape, g_q_final=None, g_qdot_last=None, g_q_trace=None, want=None, out=None, score_seed=None, watch_seed=None):
        """wbc_rollout_vjp (include/wbc.h): the reverse sweep over a recorded roll-out, everything on the device. tape: rollout_record's.
        Seeds (numpy or torch, at least one; tangent coordinates — wbc_workload.raw_to_tangent turns a raw gradient into one): g_q_final
        [B,26] at q_K, g_qdot_last [B,26], g_q_trace [K,B,26] at the state after each tick. want: names of capi.ROLLOUT_GRAD_FIELDS (None:
        d_q0 and what the configuration reads); out: caller's arrays by those names (and "grad_status", "ticks_dropped") instead.
        Returns dict(<want>..., grad_status [B] int32, ticks_dropped [B] int32); d_q0 is tangent at q_0 (wbc_workload.tangent_to_raw).
        A tape recorded with tracks (wbc_rollout_vjp_tracks): the dict also holds tracks = [dict(d_points [B,S,3], d_tangents [B,S,3],
        d_du [B]), ...], one per track in the call's order; want accepts those three names too (None: each where the track offers it —
        d_tangents for a hermite track with caller tangents alone), and out may hold "tracks": a list of dicts of the caller's arrays.
        score_seed (None: exactly the calls above; a tape recorded with tracks): wbc_rollout_vjp_scored — dict(mask: the score mask or the
        scored frames as rollout_record's `score` lists them, g_err_sq_sum, g_err_final, g_err_max [n_scored,B] (at least one), err_max_tick
        [n_scored,B] int32 (with g_err_max), q_final [B,27]: the record call's outputs). The cotangents of the scores are formed on the
        device; the state seeds become optional and, where given, the gradients are those of the summed loss.
        watch_seed (None: exactly the calls above; any tape): wbc_rollout_vjp_watched — dict(mask: the watch mask or the families as
        rollout_record's `watch` lists them, g_slack_min, g_slack_final [n_w,B], g_trace [K,n_w,B] (at least one), slack_min_tick [n_w,B]
        int32 (with g_slack_min), q_final [B,27]: the record call's outputs). The cotangents of the slacks are formed on the device at the
        taped states; the other seeds become optional and the gradients are those of the summed loss. d_trunk_box_center (where the
        configuration offers it) then also holds the watch's own box term."""
        keep = []
        c = tape.call
        inputs, B, K = c["inputs"], tape.B, tape.ticks
        tracks = c.get("tracks")
        if getattr(self, "_options", {}).get("warm_start", 0) != c["warm_start"]:
            raise capi.WbcError("rollout_vjp: option warm_start changed since the tape was recorded (the tape holds working sets only with it)")
        sseed = None
        if score_seed is not None:
            if tracks is None:
                raise capi.WbcError("score_seed: needs a tape recorded with tracks")
            sseed = {k: score_seed.get(k) for k in capi.SCORE_SEED_FIELDS}
        wseed = None if watch_seed is None else {k: watch_seed.get(k) for k in capi.WATCH_SEED_FIELDS}
        like = next((a for a in (g_q_final, g_qdot_last, g_q_trace) + tuple((sseed or {}).values()) + tuple((wseed or {}).values())
                     if a is not None), inputs["q"])
        default = lambda: self.default_rollout_grad_wants(c["mode"])
        tk = tg = None
        t_outs, arrays = [], []
        if tracks is not None:     # the names of the track outputs leave `want` / `out`; what a roll-out along tracks has no step for leaves the default
            tk, seen = self._tracks_struct(tracks, B, keep)
            tg = capi.WbcTracksGrad()
            no_step = {"d_ee_target_step"} | ({"d_trunk_target_step"} if capi.TARGET_TRUNK in seen else set())
            default = lambda: tuple(k for k in self.default_rollout_grad_wants(c["mode"]) if k not in no_step)
            track_want = None if want is None else tuple(k for k in want if k in capi.TRACK_GRAD_FIELDS)
            want = None if want is None else tuple(k for k in want if k not in capi.TRACK_GRAD_FIELDS)
            caller_tracks = None if out is None else out.get("tracks", [{}] * len(tracks))
            out = None if out is None else {k: v for k, v in out.items() if k != "tracks"}
            for j, t in enumerate(tracks):
                fields = {k: tuple(int(t["points"].shape[1]) if d == "S" else d for d in shp) for k, shp in capi.TRACK_GRAD_FIELDS.items()}
                offered = tuple(k for k in fields if k != "d_tangents" or (tk.track[j].kind == capi.TRACK_HERMITE and t.get("tangents") is not None))
                t_out, t_struct = self._grad_outs(fields, capi.WbcTrackGrad, like, B, keep,
                                                  offered if track_want is None else tuple(k for k in track_want if k in offered),
                                                  lambda: offered, None if caller_tracks is None else caller_tracks[j], extras=())
                tg.track[j] = t_struct
                t_outs.append(t_out)
                arrays += list(t_out.values())
            arrays += self._track_arrays(tracks)
        out, o = self._grad_outs(capi.ROLLOUT_GRAD_FIELDS, capi.WbcRolloutGrad, like, B, keep, want, default, out, extras=("grad_status", "ticks_dropped"))
        mem = _mem_of(list(inputs.values()) + list(out.values()) + arrays + [c["imu"], c["task_params"], g_q_final, g_qdot_last, g_q_trace] +
                      list((sseed or {}).values()) + list((wseed or {}).values()))
        f, P = np.float64, self._p
        sd = capi.WbcRolloutSeed()
        sd.g_q_final, sd.g_qdot_last = P(g_q_final, f, keep, B, NV, "g_q_final"), P(g_qdot_last, f, keep, B, NV, "g_qdot_last")
        if g_q_trace is not None:
            if tuple(g_q_trace.shape) != (K, B, NV):
                raise capi.WbcError("g_q_trace: shape %s, want (%d, %d, %d)" % (tuple(g_q_trace.shape), K, B, NV))
            sd.g_q_trace = P(g_q_trace, f, keep)
        r = capi.WbcRollout()
        r.ticks, r.mode, r.hold_ticks = K, c["mode"], 0
        r.imu = P(c["imu"], f, keep, B, 4, "imu")
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(c["task_params"], B, keep, self.device_id)
        ss = None
        if sseed is not None:
            ss = capi.WbcScoreSeed()
            m_ = score_seed.get("mask")
            ss.score_mask = int(m_) if isinstance(m_, (int, np.integer)) else sum(1 << self._target_index(f_, "score") for f_ in set(m_ or ()))
            ns = bin(ss.score_mask & 0xFFFFFFFF).count("1")
            for k_ in ("g_err_sq_sum", "g_err_final", "g_err_max"):
                setattr(ss, k_, P(sseed[k_], f, keep, ns, B, k_))
            ss.err_max_tick = P(sseed["err_max_tick"], np.int32, keep, ns, B, "err_max_tick")
            ss.q_final = P(sseed["q_final"], f, keep, B, NQS, "q_final")
        if wseed is not None:
            ws = capi.WbcWatchSeed()
            m_ = watch_seed.get("mask")
            ws.mask = int(m_) if isinstance(m_, (int, np.integer)) else sum(1 << self._slack_family(f_) for f_ in set(m_ or ()))
            nw = bin(ws.mask & 0xFFFFFFFF).count("1")
            for k_ in ("g_slack_min", "g_slack_final"):
                setattr(ws, k_, P(wseed[k_], f, keep, nw, B, k_))
            if wseed["g_trace"] is not None:
                if tuple(wseed["g_trace"].shape) != (K, nw, B):
                    raise capi.WbcError("g_trace: shape %s, want (%d, %d, %d)" % (tuple(wseed["g_trace"].shape), K, nw, B))
                ws.g_trace = P(wseed["g_trace"], f, keep)
            ws.slack_min_tick = P(wseed["slack_min_tick"], np.int32, keep, nw, B, "slack_min_tick")
            ws.q_final = P(wseed["q_final"], f, keep, B, NQS, "q_final")
            capi.check(self.lib.wbc_rollout_vjp_watched(self._h, B, C.byref(tin), tp, c["dt"], C.byref(r), C.byref(tk) if tk is not None else None,
                                                        tape.buf.data_ptr(), tape.buf.numel(), C.byref(sd), C.byref(ss) if ss is not None else None,
                                                        C.byref(ws), mem, C.byref(o), C.byref(tg) if tk is not None else None,
                                                        self._stream(mem)), self.lib)
            return out if tk is None else dict(out, tracks=t_outs)
        if tk is None:
            capi.check(self.lib.wbc_rollout_vjp(self._h, B, C.byref(tin), tp, c["dt"], C.byref(r), tape.buf.data_ptr(), tape.buf.numel(),
                                                 C.byref(sd), mem, C.byref(o), self._stream(mem)), self.lib)
            return out
        if ss is not None:
            capi.check(self.lib.wbc_rollout_vjp_scored(self._h, B, C.byref(tin), tp, c["dt"], C.byref(r), C.byref(tk), tape.buf.data_ptr(),
                                                       tape.buf.numel(), C.byref(sd), C.byref(ss), mem, C.byref(o), C.byref(tg),
                                                       self._stream(mem)), self.lib)
            return dict(out, tracks=t_outs)
        capi.check(self.lib.wbc_rollout_vjp_tracks(self._h, B, C.byref(tin), tp, c["dt"], C.byref(r), C.byref(tk), tape.buf.data_ptr(),
                                                   tape.buf.numel(), C.byref(sd), mem, C.byref(o), C.byref(tg), self._stream(mem)), self.lib)
        return dict(out, tracks=t_outs)

    def default_rollout_grad_wants(self, mode=capi.ROLLOUT_RUNNING):
        """the gradients wbc_rollout_vjp offers under the handle's configuration (names of capi.ROLLOUT_GRAD_FIELDS)"""
        return self._offered(capi.ROLLOUT_GRAD_FIELDS, self._ROLLOUT_NEEDS, mode)

    _SUMMARY = (("err_sq_sum", np.float64), ("err_max", np.float64), ("err_max_tick", np.int32), ("err_final", np.float64),
                ("first_bad_tick", np.int32), ("bad_ticks", np.int32))
    _GROUP_SUMMARY = (("group_rms", np.float64), ("group_err_max", np.float64), ("group_worst_status", np.int32),
                      ("group_bad_instances", np.int32))

    def rollout_traj(self, inputs, dt, ticks, points, n_points=None, du=0.002, ee_index=4, group_size=0, want_trace=False,
                     want_summary=True, mode=capi.ROLLOUT_RUNNING, task_params=None, trunk_target_step=None, imu=None):
        """`ticks` closed-loop ticks with the target of end effector `ee_index` following each instance's own milestone trajectory
        (wbc_rollout_traj, include/wbc.h): points [B, S, 3], n_points [B] int32 (None: S milestones everywhere), du [B] or one number
        (parameter advance per tick, sim3.py:225). Tick k's target is wbc_workload.traj_targets(points, n_points, du, k). Returns
        rollout()'s dict (grip_trace only with want_trace) plus, with want_summary, the per-instance arrays err_sq_sum, err_max,
        err_max_tick, err_final, first_bad_tick, bad_ticks [B] and, with group_size = M > 0 (B % M == 0), group_rms, group_err_max,
        group_worst_status, group_bad_instances [B / M] — all reduced on the device."""
        keep = []
        du_arr = None if np.isscalar(du) else du
        mem = _mem_of(list(inputs.values()) + [points, n_points, du_arr, trunk_target_step, imu, task_params])
        q = inputs.get("q")
        B = self._batch_of(q)
        shape = tuple(getattr(points, "shape", ()))
        if len(shape) != 3 or shape[0] != B or shape[2] != 3 or not 2 <= shape[1] <= capi.MAX_TRAJ_POINTS:
            raise capi.WbcError("points: shape %s, want (%d, S, 3) with 2 <= S <= %d" % (shape, B, capi.MAX_TRAJ_POINTS))
        S = int(shape[1])
        if not 0 <= int(ee_index) < capi.NEE:
            raise capi.WbcError("ee_index = %d outside [0, %d]" % (ee_index, capi.NEE - 1))
        M = self._check_ticks_groups(B, ticks, group_size)
        f = np.float64
        P = self._p
        t = capi.WbcTrajectory()
        t.max_points, t.ee_index = S, int(ee_index)
        t.points = P(points, f, keep, B, S * 3, "points")
        t.n_points = P(n_points, np.int32, keep, B, 1, "n_points")
        if du_arr is None:
            t.du_all = float(du)
        else:
            t.du = P(du_arr, f, keep, B, 1, "du")
        out, r = self._rollout_base(inputs, B, keep, ticks, mode, 0, None, trunk_target_step, imu, want_trace)
        sm = None
        if want_summary:
            sm = capi.WbcRolloutSummary()
            sm.group_size = M
            for name, dtype in self._SUMMARY + (self._GROUP_SUMMARY if M > 0 else ()):
                out[name] = self._alloc(q, (B // M if name.startswith("group_") else B,), dtype)
                setattr(sm, name, P(out[name], dtype, keep))
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        capi.check(self.lib.wbc_rollout_traj(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), C.byref(t),
                                             C.byref(sm) if sm is not None else None, mem, self._stream(mem)), self.lib)
        return out

    _TRACK_KEYS = ("target", "points", "kind", "tangents", "n_points", "du")
    _KINDS = {"linear": capi.TRACK_LINEAR, "hermite": capi.TRACK_HERMITE, capi.TRACK_LINEAR: capi.TRACK_LINEAR, capi.TRACK_HERMITE: capi.TRACK_HERMITE}
    _FRAME_SCORES = (("err_sq_sum", np.float64), ("err_max", np.float64), ("err_final", np.float64), ("err_max_tick", np.int32))
    _INSTANCE_SCORES = (("first_bad_tick", np.int32), ("bad_ticks", np.int32))

    @staticmethod
    def _target_index(t, what):
        if isinstance(t, str) and t == "trunk":
            return capi.TARGET_TRUNK
        if isinstance(t, (str, bool)) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) <= capi.TARGET_TRUNK:
            raise capi.WbcError("%s: %r is neither 'trunk' nor an end effector index 0..%d" % (what, t, capi.NEE - 1))
        return int(t)

    _SLACK_FAMILIES = {"com": capi.SLACK_COM, "trunk_z": capi.SLACK_TRUNK_Z, "trunk_ang": capi.SLACK_TRUNK_ANG, "joint": capi.SLACK_JOINT}
    _WATCH_ROWS = (("slack_min", np.float64), ("slack_final", np.float64), ("slack_min_tick", np.int32), ("slack_min_which", np.int32),
                   ("neg_ticks", np.int32), ("first_neg_tick", np.int32))
    _WATCH_GROUPS = (("group_min", np.float64), ("group_neg_instances", np.int32))

    @classmethod
    def _slack_family(cls, f):
        if isinstance(f, str):
            if f not in cls._SLACK_FAMILIES:
                raise capi.WbcError("watch: %r is none of %s" % (f, ", ".join(cls._SLACK_FAMILIES)))
            return cls._SLACK_FAMILIES[f]
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= int(f) < capi.N_SLACK:
            raise capi.WbcError("watch: %r is neither a family name (%s) nor an index 0..%d" % (f, ", ".join(cls._SLACK_FAMILIES), capi.N_SLACK - 1))
        return int(f)

    def state_slack(self, q, trunk_box_center=None, model_id=None, want_components=False):
        """Slack of the reference's constraint quantities at q [B, 27] (wbc_state_slack, include/wbc.h; restated in numpy by
        wbc_workload.state_slack): dict(slack [B, 4] float64, which [B, 4] int32[, components [B, 12]]), families in the order CoM box,
        trunk z, trunk angles, joint range; >= 0 inside, < 0 outside, evaluated whether or not the configuration enforces the constraint.
        trunk_box_center [B, 4] (None: the two trunk families come back NaN / -1)."""
        keep = []
        mem = _mem_of([q, trunk_box_center, model_id])
        B = self._batch_of(q)
        out = dict(slack=self._alloc(q, (B, capi.N_SLACK)), which=self._alloc(q, (B, capi.N_SLACK), np.int32))
        if want_components:
            out["components"] = self._alloc(q, (B, capi.N_SLACK_COMPONENTS))
        o = capi.WbcSlackOut()
        for k, v in out.items():
            setattr(o, k, self._p(v, np.int32 if k == "which" else np.float64, keep))
        f = np.float64
        capi.check(self.lib.wbc_state_slack(self._h, B, self._p(q, f, keep), self._p(trunk_box_center, f, keep, B, 4, "trunk_box_center"),
                                            self._p(model_id, np.int32, keep, B, 1, "model_id"), mem, C.byref(o), self._stream(mem)), self.lib)
        return out

    def state_slack_grad(self, q, trunk_box_center=None, g_slack=None, g_components=None, model_id=None):
        """The cotangent of state_slack's outputs (wbc_state_slack_vjp, include/wbc.h; restated in numpy by wbc_workload.slack_gradients):
        g_slack [B, 4] = dL/d slack and / or g_components [B, 12] = dL/d components -> dict(d_q [B, 26] in tangent coordinates at q
        (wbc_workload.tangent_to_raw), d_trunk_box_center [B, 4], which [B, 4] int32: the component each family's cotangent went to,
        state_slack's `which`; grad_status [B] int32). One kernel launch, nothing allocated by the library."""
        keep = []
        mem = _mem_of([q, trunk_box_center, model_id, g_slack, g_components])
        B = self._batch_of(q)
        out = {k: self._alloc(q, (B,) + shp) for k, shp in capi.SLACK_GRAD_FIELDS.items()}
        out["which"] = self._alloc(q, (B, capi.N_SLACK), np.int32)
        out["grad_status"] = self._alloc(q, (B,), np.int32)
        o = capi.WbcSlackGrad()
        for k, v in out.items():
            setattr(o, k, self._p(v, np.int32 if k in ("which", "grad_status") else np.float64, keep))
        f, P = np.float64, self._p
        capi.check(self.lib.wbc_state_slack_vjp(self._h, B, P(q, f, keep), P(trunk_box_center, f, keep, B, 4, "trunk_box_center"),
                                                P(model_id, np.int32, keep, B, 1, "model_id"), P(g_slack, f, keep, B, capi.N_SLACK, "g_slack"),
                                                P(g_components, f, keep, B, capi.N_SLACK_COMPONENTS, "g_components"), mem, C.byref(o),
                                                self._stream(mem)), self.lib)
        return out

    def rollout_watch(self, inputs, dt, ticks, watch=("com", "trunk_z", "trunk_ang", "joint"), tracks=None, score=(), group_size=0,
                      want_trace=False, mode=capi.ROLLOUT_RUNNING, task_params=None, trunk_target_step=None, imu=None,
                      ee_target_step=None, hold_ticks=0):
        """rollout_tracks (with tracks) or rollout (tracks=None: ee_target_step and hold_ticks as there) with the slack families in `watch`
        ("com", "trunk_z", "trunk_ang", "joint" or 0..3) evaluated after every tick on the state the tick left (wbc_rollout_watch,
        include/wbc.h). Returns that call's dict plus, rows in increasing family order, slack_min, slack_final [n_w, B], slack_min_tick,
        slack_min_which, neg_ticks, first_neg_tick [n_w, B] int32, with want_trace slack_trace [ticks + hold_ticks, n_w, B], and with
        group_size = M > 0 slack_group_min, slack_group_neg_instances [n_w, B / M] — all reduced on the device
        (wbc_workload.watch_summary restates the reduction over ticks). An empty `watch` is the call without a watch."""
        fams = sorted({self._slack_family(f_) for f_ in watch})
        if len(fams) != len(list(watch)):
            raise capi.WbcError("watch: a family is listed twice")
        if tracks is None and len(list(score)):
            raise capi.WbcError("score: needs tracks")
        return self._rollout_tracks(inputs, dt, ticks, tracks, score, group_size, want_trace, mode, task_params, trunk_target_step, imu,
                                    fams, ee_target_step, hold_ticks)

    def rollout_tracks(self, inputs, dt, ticks, tracks, score=(), group_size=0, want_trace=False, mode=capi.ROLLOUT_RUNNING,
                       task_params=None, trunk_target_step=None, imu=None):
        """`ticks` closed-loop ticks with several targets following per-instance tracks (wbc_rollout_tracks, include/wbc.h). tracks: a list of
        dicts with target ("trunk" or an end effector index 0..4, each at most once), points [B, S, 3], and optionally kind ("linear",
        the default, or "hermite"), tangents [B, S, 3] (hermite only; None: wbc_workload.spline_tangents), n_points [B] int32 (None: S),
        du [B] or one number (default 0.002). Tick k's target is wbc_workload.track_targets(points, n_points, du, k, kind, tangents).
        score: the frames ("trunk" or 0..4) scored against their target of the tick, followed or constant. Returns rollout()'s dict
        (grip_trace only with want_trace) plus trunk_target [B, 3] (with a trunk target among the inputs) and, with frames to score,
        err_sq_sum, err_max, err_final, err_max_tick [n_scored, B] (frames in increasing index order, the trunk last), first_bad_tick,
        bad_ticks [B], with want_trace trace [ticks, n_scored, B, 3], and with group_size = M > 0 group_rms, group_err_max
        [n_scored, B / M], group_worst_status, group_bad_instances [B / M] — all reduced on the device."""
        return self._rollout_tracks(inputs, dt, ticks, tracks, score, group_size, want_trace, mode, task_params, trunk_target_step, imu)

    def _track_arrays(self, tracks):
        """the arrays of a list of track dicts (for _mem_of), after the check of each dict's keys"""
        arrays = []
        for i, t in enumerate(tracks):
            if not isinstance(t, dict) or set(t) - set(self._TRACK_KEYS) or "target" not in t or "points" not in t:
                raise capi.WbcError("tracks[%d]: want a dict with target, points and optionally kind, tangents, n_points, du" % i)
            arrays += [t["points"], t.get("tangents"), t.get("n_points"), None if np.isscalar(t.get("du", 0.002)) else t.get("du")]
        return arrays

    def _tracks_struct(self, tracks, B, keep):
        """-> (WbcTracks of the list of dicts, the set of followed targets)"""
        f = np.float64
        P = self._p
        tk = capi.WbcTracks()
        tk.n_tracks = len(tracks)
        seen = set()
        for i, t in enumerate(tracks):
            who = "tracks[%d]" % i
            c = tk.track[i]
            c.target = self._target_index(t["target"], who + ".target")
            if c.target in seen:
                raise capi.WbcError("%s.target: %r is followed twice" % (who, t["target"]))
            seen.add(c.target)
            kind = t.get("kind", "linear")
            if not isinstance(kind, (str, int)) or kind not in self._KINDS:
                raise capi.WbcError("%s.kind: %r is neither 'linear' nor 'hermite'" % (who, kind))
            c.kind = self._KINDS[kind]
            shape = tuple(getattr(t["points"], "shape", ()))
            if len(shape) != 3 or shape[0] != B or shape[2] != 3 or not 2 <= shape[1] <= capi.MAX_TRAJ_POINTS:
                raise capi.WbcError("%s.points: shape %s, want (%d, S, 3) with 2 <= S <= %d" % (who, shape, B, capi.MAX_TRAJ_POINTS))
            S = int(shape[1])
            c.max_points = S
            c.points = P(t["points"], f, keep, B, S * 3, who + ".points")
            tg = t.get("tangents")
            if tg is not None:
                if c.kind == capi.TRACK_LINEAR:
                    raise capi.WbcError("%s.tangents: a linear track has no tangents" % who)
                if tuple(getattr(tg, "shape", ())) != shape:
                    raise capi.WbcError("%s.tangents: shape %s, want %s" % (who, tuple(getattr(tg, "shape", ())), shape))
                c.tangents = P(tg, f, keep, B, S * 3, who + ".tangents")
            c.n_points = P(t.get("n_points"), np.int32, keep, B, 1, who + ".n_points")
            du = t.get("du", 0.002)
            if np.isscalar(du):
                c.du_all = float(du)
            else:
                c.du = P(du, f, keep, B, 1, who + ".du")
        return tk, seen

    def _scores_struct(self, out, like, frames, B, K, M, want_trace, keep):
        """allocates the scores of `frames` into `out` -> the WbcTrackScores that points at them (None: nothing to score)"""
        ns = len(frames)
        if not ns:
            return None
        sc = capi.WbcTrackScores()
        sc.group_size = M
        for fr in frames:
            sc.score_mask |= 1 << fr
        spec = [(n, (ns, B), d) for n, d in self._FRAME_SCORES] + [(n, (B,), d) for n, d in self._INSTANCE_SCORES]
        if want_trace:
            spec.append(("trace", (K, ns, B, 3), np.float64))
        if M > 0:
            spec += [(n, (ns, B // M) if n in ("group_rms", "group_err_max") else (B // M,), d) for n, d in self._GROUP_SUMMARY]
        for name, shape, dtype in spec:
            out[name] = self._alloc(like, shape, dtype)
            setattr(sc, name, self._p(out[name], dtype, keep))
        return sc

    def _watch_struct(self, out, like, fams, B, total, M, want_trace, keep):
        """allocates the watch's results of the families `fams` into `out` -> the WbcSlackWatch that points at them (None: no family)"""
        nw = len(fams)
        if not nw:
            return None
        wt = capi.WbcSlackWatch()
        wt.group_size = M
        for fam in fams:
            wt.mask |= 1 << fam
        for name, dtype in self._WATCH_ROWS:
            out[name] = self._alloc(like, (nw, B), dtype)
            setattr(wt, name, self._p(out[name], dtype, keep))
        if want_trace:
            out["slack_trace"] = self._alloc(like, (total, nw, B))
            wt.trace = self._p(out["slack_trace"], np.float64, keep)
        if M > 0:
            for name, dtype in self._WATCH_GROUPS:
                out["slack_" + name] = self._alloc(like, (nw, B // M), dtype)
                setattr(wt, name, self._p(out["slack_" + name], dtype, keep))
        return wt

    def _rollout_tracks(self, inputs, dt, ticks, tracks, score, group_size, want_trace, mode, task_params, trunk_target_step, imu,
                        watch=None, ee_target_step=None, hold_ticks=0):
        """the body of rollout_tracks and rollout_watch. watch: None (wbc_rollout_tracks) or the sorted family indices (wbc_rollout_watch;
        tracks may then be None, and ee_target_step / hold_ticks are passed on)"""
        keep = []
        tracks = [] if (tracks is None and watch is not None) else list(tracks)
        if not (0 if watch is not None else 1) <= len(tracks) <= capi.MAX_TRACKS:
            raise capi.WbcError("tracks: %d given, want 1..%d" % (len(tracks), capi.MAX_TRACKS))
        arrays = [ee_target_step] + self._track_arrays(tracks)
        mem = _mem_of(list(inputs.values()) + arrays + [trunk_target_step, imu, task_params])
        q = inputs.get("q")
        B = self._batch_of(q)
        M = self._check_ticks_groups(B, ticks, group_size)
        tk, seen = self._tracks_struct(tracks, B, keep)
        if capi.TARGET_TRUNK in seen and trunk_target_step is not None:
            raise capi.WbcError("trunk_target_step: not together with a trunk track")
        frames = sorted({self._target_index(s_, "score") for s_ in score})
        if len(frames) != len(list(score)):
            raise capi.WbcError("score: a frame is listed twice")
        need_trunk = capi.TARGET_TRUNK in seen or capi.TARGET_TRUNK in frames
        if need_trunk and (inputs.get("trunk_target") is None or inputs.get("prev_trunk_target") is None):
            raise capi.WbcError("a trunk track or a scored trunk needs the inputs trunk_target and prev_trunk_target")
        K, H = int(ticks), int(hold_ticks)
        if H < 0:
            raise capi.WbcError("hold_ticks = %d, want >= 0" % H)
        out, r = self._rollout_base(inputs, B, keep, K, mode, H, ee_target_step, trunk_target_step, imu, want_trace)
        if inputs.get("trunk_target") is not None and tracks:
            out["trunk_target"] = self._alloc(q, (B, 3))
            tk.trunk_target_final = self._p(out["trunk_target"], np.float64, keep)
        sc = self._scores_struct(out, q, frames, B, K, M, want_trace, keep)
        tin = self._tick_in(inputs, keep, B)
        tp = _task_params(task_params, B, keep, self.device_id)
        sc_ref = C.byref(sc) if sc is not None else None
        if watch is None:
            capi.check(self.lib.wbc_rollout_tracks(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), C.byref(tk), sc_ref, mem, self._stream(mem)), self.lib)
            return out
        wt = self._watch_struct(out, q, watch, B, K + H, M, want_trace, keep)
        capi.check(self.lib.wbc_rollout_watch(self._h, B, C.byref(tin), tp, float(dt), C.byref(r), C.byref(tk) if tracks else None, sc_ref,
                                              C.byref(wt) if wt is not None else None, mem, self._stream(mem)), self.lib)
        return out

    def integrate(self, q, v, dt, model_id=None):
        """pin.integrate(model, q, v * dt) for every instance."""
        keep = []
        mem = _mem_of([q, v, model_id])
        B = self._batch_of(q)
        qn = self._alloc(q, (B, NQS))
        f = np.float64
        P = self._p
        capi.check(self.lib.wbc_integrate(self._h, B, P(q, f, keep), P(v, f, keep, B, NV, "v"), P(model_id, np.int32, keep, B, 1, "model_id"),
                                           float(dt), mem, P(qn, f, keep), self._stream(mem)), self.lib)
        return qn

    # ---- setInitialState for B robots
    def warm_up(self, q0, model_id=None, dt=0.002, ticks_per_segment=1000, foot_radius=0.0, configure=True):
        """``RobotModel.setInitialState`` (reference Robot_Wrapper4.py:196-351) for every instance of a batch: from q0 [B,27]
        (the reference starts from pin.neutral with the joints clamped to their upper limits, :199-208) the six Cartesian
        tasks + Tikhonov posture drag the feet and the gripper along straight lines to the crouched stance — 2 x
        ticks_per_segment bounds-only QPs per robot, ONE wbc_rollout call (mode WARMUP) for the whole batch — then the base
        orientation is reset and the trunk height set from the foot heights (:328-338).
        configure=True puts the warm-up's own switch set on the handle (setTasks(all True), no constraints, default weights: :272)
        and leaves it there. Host arrays in, dict(q [B,27], status, iters, start, goal) out."""
        import wbc_model
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        B = self._batch_of(q0, "q0")
        mid = None if model_id is None else np.ascontiguousarray(model_id, dtype=np.int32)
        if configure:
            for i, m in enumerate(self.models):
                self.configure(wbc_model.make_config(m, Trunk=True, FR=True, FL=True, RR=True, RL=True, Grip=True, Joint=True), i)
        f = self.fk(q0, mid, want=("oMf",))["oMf"]                        # updateState(q, feedback=False), :211
        pos, rot = f[:, :, 9:12], f[:, :, 0:9]
        ee, trunk = pos[:, capi.FR_EE0:capi.FR_EE0 + 5].copy(), pos[:, capi.FR_TRUNK].copy()
        Rt = rot[:, capi.FR_TRUNK].reshape(B, 3, 3)
        Ree = rot[:, capi.FR_EE0:capi.FR_EE0 + 5].reshape(B, 5, 3, 3)
        goal = ee.copy()                                                   # :238-262
        goal[:, :4, 0] = pos[:, capi.FR_HIP0:capi.FR_HIP0 + 4, 0]          # feet under their hips ...
        goal[:, :4, 2] *= 0.9                                              # ... and 10 % closer to the trunk (multiplier_F / _R)
        goal[:, 4, 2] = pos[:, capi.FR_ARM_BASE, 2]                        # gripper: height of oMi[arm_base_id] (G_base, :37, :253 — a constructor
        goal[:, 4, 0] = pos[:, capi.FR_HIP0, 0]                            # argument of its own, not the fifth hip_waist name), x of the FR hip
        goal[:, 4, 0] *= 1.1                                               # multiplier_G = diag(1.1, 1, 1.5)
        goal[:, 4, 2] *= 1.5
        n = int(ticks_per_segment)
        d = dict(q=q0, ee_target=ee, prev_ee_target=ee.copy(), trunk_target=trunk, prev_trunk_target=trunk.copy(),
                 ee_ref_rot=Ree.reshape(B, 5, 9).copy(),                   # R* = from_euler(as_euler(R_EE)) = R_EE (:222-226)
                 ee_prev_rot=np.einsum("bji,bejk->beik", Rt, Ree).reshape(B, 5, 9),     # prev_EE_CoM_rot = R_trunk' R_EE (:219)
                 trunk_ref_euler=np.stack([np.arctan2(Rt[:, 2, 1], Rt[:, 2, 2]), -np.arcsin(np.clip(Rt[:, 2, 0], -1, 1)),
                                           np.arctan2(Rt[:, 1, 0], Rt[:, 0, 0])], axis=1),
                 trunk_prev_rot=np.zeros((B, 9)))                          # old_ref_trunk_rot_matrix = zeros before initialiseWBC (:150)
        if mid is not None:
            d["model_id"] = mid
        warm = getattr(self, "_options", {}).get("warm_start", 0)
        self.set_option("warm_start", 0)                                   # the reference builds a fresh QP object every iteration (:320): cold
        try:
            ro = self.rollout(d, dt, n, ee_target_step=(goal - ee) / n, want_trace=False, mode=capi.ROLLOUT_WARMUP, hold_ticks=n)
        finally:
            self.set_option("warm_start", warm)
        q = ro["q"].copy()
        q[:, 3:6] = 0.0                                                    # "reset base orientation" (:328-330): x, y, z of the quaternion
        feet_z = self.fk(q, mid, want=("oMf",))["oMf"][:, capi.FR_EE0:capi.FR_EE0 + 4, 11]
        q[:, 2] = -feet_z.mean(axis=1) + foot_radius                       # :336-337
        return dict(q=q, status=ro["status"], iters=ro["iters"], start=ee, goal=goal)
