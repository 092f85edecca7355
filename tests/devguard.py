"""Guarded device buffers for the in-place (WBC_MEM_DEVICE) tests: tests/test_gpu_device_inplace.py.

Every array handed to the library is the live part of one flat torch allocation: G guard rows, the live rows, G guard rows, a "row" being
everything behind the leading dimension. G = 5 is odd on purpose: the live view of a [B][27] float64 array starts 1080 bytes into the
allocation — naturally aligned, which is all the C ABI promises, and no better. Output guards hold one fixed bit pattern per dtype and are
compared as bytes after the call; input guards hold either rows of ANOTHER valid batch or NaN rows, and every input allocation (guards and
live rows) must come back byte for byte. All calls run on a non-default torch stream (Session.run)."""
import numpy as np
import torch

G = 5
# one fixed bit pattern per dtype: a quiet NaN with a payload, negative constants
_PATTERN = {np.dtype(np.float64): np.array([0x7FF8DEADBEEF5A5A], dtype=np.uint64).view(np.float64)[0],
            np.dtype(np.int32): np.int32(-1515870811), np.dtype(np.int64): np.int64(-6510615555426900571)}
_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


def _bytes(t):
    return t.cpu().numpy().reshape(-1).view(np.uint8).copy()


class Guarded:
    """one flat device allocation [G rows | live | G rows]; .live is the contiguous view the library gets"""

    def __init__(self, host_full, shape):
        self.shape = tuple(shape)
        self.row = int(np.prod(self.shape[1:], dtype=np.int64))
        self.n = int(self.shape[0]) * self.row
        assert host_full.ndim == 1 and host_full.size == self.n + 2 * G * self.row
        self.flat = torch.from_numpy(np.ascontiguousarray(host_full)).cuda()
        self.live = self.flat[G * self.row:G * self.row + self.n].view(self.shape)
        assert self.live.is_contiguous() and self.live.data_ptr() == self.flat.data_ptr() + G * self.row * host_full.itemsize
        self.before = host_full.view(np.uint8).copy()

    def guards(self):
        b = _bytes(self.flat)
        k = G * self.row * self.flat.element_size()
        return b[:k], b[len(b) - k:]

    def unchanged(self):
        return np.array_equal(_bytes(self.flat), self.before)


def guarded_input(live, guard_rows=None):
    """live: numpy [B, ...]; guard_rows: numpy [2 G, ...] of the same trailing shape and dtype (rows of another valid batch), or None: NaN rows
    (float64 only)."""
    live = np.ascontiguousarray(live)
    row_shape = live.shape[1:]
    if guard_rows is None:
        assert live.dtype == np.float64
        guard_rows = np.full((2 * G,) + row_shape, np.nan)
    guard_rows = np.ascontiguousarray(guard_rows, dtype=live.dtype)
    assert guard_rows.shape == (2 * G,) + row_shape, (guard_rows.shape, live.shape)
    full = np.concatenate([guard_rows[:G].reshape(-1), live.reshape(-1), guard_rows[G:].reshape(-1)])
    return Guarded(full, live.shape)


def guarded_output(shape, dtype):
    dtype = np.dtype(dtype)
    row = int(np.prod(tuple(shape)[1:], dtype=np.int64))
    full = np.full(int(shape[0]) * row + 2 * G * row, _PATTERN[dtype], dtype=dtype)
    return Guarded(full, shape)


class Session:
    """The guarded buffers of one call: inputs (snapshot, must come back unchanged), outputs (pattern guards, must come back intact).
    `alloc` is the WbcBatch allocator hook: every output a wrapper allocates itself becomes a guarded buffer of this session.
    mode: "exact" (plain exact-size tensors, no guards), "other" (input guards = rows of another batch), "nan" (NaN input guards where
    `nan_ok` names the array, the other batch elsewhere)."""

    def __init__(self, mode, stream):
        assert mode in ("exact", "other", "nan")
        self.mode, self.stream = mode, stream
        self.inputs, self.outputs = {}, []

    def put(self, name, live, other, nan_ok=True):
        """-> the device tensor for input `name`; other: [>= 2 G, ...] rows of another valid batch"""
        if live is None:
            return None
        live = np.ascontiguousarray(live)
        if self.mode == "exact":
            return torch.from_numpy(live.copy()).cuda()
        use_nan = self.mode == "nan" and nan_ok and live.dtype == np.float64
        g = guarded_input(live, None if use_nan else np.asarray(other)[:2 * G])
        self.inputs[name] = g
        return g.live

    def put_all(self, d, other, nan_ok=True):
        return {k: self.put(k, v, other[k], nan_ok) for k, v in d.items()}

    def out(self, shape, dtype=np.float64):
        """-> a device tensor for an output the test passes itself"""
        if self.mode == "exact":
            return torch.empty(tuple(shape), dtype=_TORCH[np.dtype(dtype)], device="cuda")
        g = guarded_output(shape, dtype)
        self.outputs.append(g)
        return g.live

    def alloc(self, like, shape, dtype=np.float64):
        return self.out(shape, dtype)

    def run(self, fn):
        """fn() on the side stream; synchronised before anything is read"""
        with torch.cuda.stream(self.stream):
            res = fn()
        self.stream.synchronize()
        return res

    def check(self, what, aliased=()):
        """output guards intact, every input allocation byte-identical to its state before the call (`aliased`: inputs deliberately
        aliased to an output: their guards must still be intact)"""
        for i, g in enumerate(self.outputs):
            lo, hi = g.guards()
            k = len(lo)
            assert np.array_equal(lo, g.before[:k]), "%s: output %d %s: rows BEFORE the array were written" % (what, i, g.shape)
            assert np.array_equal(hi, g.before[len(g.before) - k:]), "%s: output %d %s: rows BEHIND the array were written" % (what, i, g.shape)
        for name, g in self.inputs.items():
            if name in aliased:
                lo, hi = g.guards()
                k = len(lo)
                assert np.array_equal(lo, g.before[:k]) and np.array_equal(hi, g.before[len(g.before) - k:]), "%s: guards of aliased %s were written" % (what, name)
            else:
                assert g.unchanged(), "%s: input %s was written" % (what, name)


def to_host(res):
    """dict / tuple / tensor of device results -> numpy copies"""
    if isinstance(res, dict):
        return {k: to_host(v) for k, v in res.items()}
    if isinstance(res, (tuple, list)):
        return tuple(to_host(v) for v in res)
    return None if res is None else res.cpu().numpy().copy()


def same_bytes(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
