"""Host-side mirror of the ExponentialUtilities.jl Krylov API over the C ABI (libexpv_mi.so).

Julia is not available in this image, so the host language above the C ABI is Python; names,
argument meaning, defaults and error behaviour follow the reference so the parity tests read like
the reference's own tests:

    reference (Julia)                              here
    ---------------------------------------------  -----------------------------------------
    KrylovSubspace{T,U}(n, maxiter, augmented)     KrylovSubspace(T, U, n, maxiter, augmented)
    arnoldi(A, b; m, ishermitian, tol, iop)        arnoldi(A, b, m=, ishermitian=, tol=, iop=)
    arnoldi!(Ks, A, b; ...) / lanczos!(Ks, A, b)   arnoldi_(Ks, A, b, ...) / lanczos_(Ks, A, b, ...)
    expv(t, A, b; mode, ...) / expv!(w, t, Ks)     expv(t, A, b, mode=, ...) / expv_(w, t, Ks)
    phiv(t, A, b, k; ...) / phiv!(w, t, Ks, k)     phiv(t, A, b, k, ...) / phiv_(w, t, Ks, k, ...)
    expv_timestep / phiv_timestep (! forms)        expv_timestep / phiv_timestep (+ trailing _)
    kiops(tau_out, A, u; ...)                      kiops(tau_out, A, u, ...)

Vectors may be numpy arrays (staged through HBM by the library) or torch CUDA tensors / DeviceArray
(used in place, nothing crosses PCIe).  Every O(n) operation runs in the HIP kernels of csrc/.
"""
import ctypes as C
import math
import os
import weakref

import numpy as np

from . import _lib as L

__all__ = [
    "Context", "default_context", "MIOperator", "DeviceArray", "KrylovSubspace", "arnoldi", "arnoldi_",
    "lanczos_", "expv", "expv_", "phiv", "phiv_", "expv_timestep", "expv_timestep_", "phiv_timestep",
    "phiv_timestep_", "kiops", "timestep_caches", "expv_batch", "expv_batch_multi", "RcclComm", "rccl_available", "rccl_unique_id", "ExpvMIError", "DimensionMismatch", "host_expm",
    "exponential", "exponential_", "mul_", "phi", "phi_", "balance_", "host_gebal",
    "host_phiv_dense", "host_symtridiag_expcol", "host_symtridiag_exp_last", "host_pattern_info", "host_dia_pattern", "host_rcm", "host_patch_order", "clear_operator_cache", "plan_cache",
    "expv_taylor", "expv_taylor_", "expv_taylor_block", "expv_taylor_block_", "expv_taylor_grid", "expv_taylor_grid_", "host_taylor_grid_plan", "phiv_taylor", "phiv_taylor_", "host_taylor_theta", "host_taylor_params",
    "expv_taylor_realop", "expv_taylor_realop_",
    "expv_taylor_power", "expv_taylor_power_", "host_taylor_params_power", "host_normest_signs",
]

ExpvMIError = L.ExpvMIError


class DimensionMismatch(ValueError):
    """Julia's DimensionMismatch (arnoldi.jl:217-218) -- raised for status 1."""


def _check(code, ctx=None):
    if code == 0:
        return
    try:
        L.check(code, ctx)
    except L.ExpvMIError as e:
        if e.code == 1:
            raise DimensionMismatch(str(e)) from None
        if e.code == 3:
            raise AssertionError(str(e)) from None
        if e.code == 8:
            raise IndexError(str(e)) from None
        raise


# ---------------------------------------------------------------------------------------------
# context and raw device memory
# ---------------------------------------------------------------------------------------------
class Context:
    """One GPU + one HIP stream (expv_mi_ctx_create).  ``stream``: None -- the library creates a private non-blocking stream -- or a
    stream of the caller's (a torch.cuda.Stream, or a hipStream_t as an integer) that the library launches on and never destroys.
    The null / legacy stream (handle 0, e.g. torch.cuda.default_stream()) cannot be adopted: the C ABI reads a NULL handle as
    "create a private stream", and the caller would believe the library ordered with a stream it is not on."""


    def __init__(self, device=None, stream=None, async_outputs=False):
        sptr = None
        if stream is not None:
            handle = getattr(stream, "cuda_stream", stream)
            if not handle:
                raise ValueError("Context(stream=...): the null / legacy stream (handle 0, e.g. torch.cuda.default_stream()) cannot be "
                                 "adopted -- the library would silently work on a stream of its own.  Pass a stream you created "
                                 "(torch.cuda.Stream()), or stream=None for a private stream of the library's.")
            sptr = C.c_void_p(int(handle))
        lib = L.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        h = C.c_void_p()
        _check(lib.expv_mi_ctx_create(int(device), sptr, C.byref(h)))
        self._h = h
        self.device = int(device)
        self._stream_keepalive = stream
        self._finalizer = weakref.finalize(self, lib.expv_mi_ctx_destroy, h)
        # async_outputs: device-resident results are stream-ordered (valid after ctx.sync() or for later work on
        # the context's stream) instead of complete when a call returns
        self._async_outputs = bool(async_outputs)
        if async_outputs:
            _check(lib.expv_mi_ctx_set_async_outputs(h, 1))

    def sync(self):
        _check(L.load().expv_mi_ctx_sync(self._h), self._h)

    def set_async_outputs(self, on=True):
        """Device-resident results stream-ordered (True) or complete on return (False, the C-ABI default)."""
        _check(L.load().expv_mi_ctx_set_async_outputs(self._h, int(bool(on))), self._h)
        self._async_outputs = bool(on)

    def set_option(self, name, value):
        """Engine option of this context by name (expv_mi_ctx_set_option; see include/expv_mi.h for the list)."""
        _check(L.load().expv_mi_ctx_set_option(self._h, name.encode(), int(value)), self._h)

    def get_option(self, name):
        v = C.c_int64(0)
        _check(L.load().expv_mi_ctx_get_option(self._h, name.encode(), C.byref(v)), self._h)
        return int(v.value)

    def selftest(self):
        """Device self-test of the VALU lane exchanges (expv_mi_ctx_selftest): mismatch counts per class, all zero when healthy."""
        out = (C.c_int64 * 8)()
        _check(L.load().expv_mi_ctx_selftest(self._h, out), self._h)
        return tuple(int(x) for x in out)

    def counters(self):
        """Cumulative counters of the context (expv_mi_ctx_counters)."""
        out = (C.c_int64 * 8)()
        _check(L.load().expv_mi_ctx_counters(self._h, out), self._h)
        keys = ("krylov_steps", "factorisations", "pipeline", "overlapped", "redo_serial", "redo_wave_off", "op_applies", "h_by_copy")
        return dict(zip(keys, (int(v) for v in out)))

    def last_path(self):
        """Step form of the most recent factorisation on this context (expv_mi_ctx_last_path): {"path": names of L.PATH_FLAGS,
        "fa2_pipelined", "real_operator"} -- what expv.last_stats reports, for arnoldi_ / lanczos_ and the drivers too."""
        f = C.c_int32(0)
        _check(L.load().expv_mi_ctx_last_path(self._h, C.byref(f)), self._h)
        return {"path": [k for k, v in L.PATH_FLAGS.items() if f.value & v], "fa2_pipelined": bool(f.value & L.PATH_FA2_PIPELINED),
                "real_operator": bool(f.value & L.PATH_REAL_OPERATOR)}

    def set_pipeline_overlap(self, on=True):
        """Banded pipeline: consecutive Krylov steps on two streams (default) or one launch after the other."""
        _check(L.load().expv_mi_ctx_set_pipeline_overlap(self._h, int(bool(on))), self._h)

    # per-kernel timing for bench.py's roofline leg
    def prof_enable(self, on=True):
        L.load().expv_mi_prof_enable(self._h, int(bool(on)))

    def prof_reset(self):
        _check(L.load().expv_mi_prof_reset(self._h), self._h)

    def prof_get(self):
        out = {}
        for name, kid in L.KERNEL_IDS.items():
            n, ms = C.c_int64(0), C.c_double(0.0)
            _check(L.load().expv_mi_prof_get(self._h, kid, C.byref(n), C.byref(ms)), self._h)
            if n.value:
                out[name] = {"launches": int(n.value), "total_ms": float(ms.value)}
        return out


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


class DeviceArray:
    """A column-major HBM array owned by the library (expv_mi_malloc); the Julia shim's MIVector/MIMatrix."""

    def __init__(self, shape, dtype, ctx=None):
        self.ctx = ctx or default_context()
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(L.load().expv_mi_malloc(self.ctx._h, nbytes, C.byref(p)), self.ctx._h)
        self.ptr = p.value
        self.nbytes = nbytes
        self._finalizer = weakref.finalize(self, L.load().expv_mi_free, self.ctx._h, p)

    @classmethod
    def from_host(cls, a, ctx=None):
        a = np.asfortranarray(a)
        d = cls(a.shape, a.dtype, ctx)
        _check(L.load().expv_mi_memcpy_h2d(d.ctx._h, d.ptr, a.ctypes.data, a.nbytes), d.ctx._h)
        return d

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype, order="F")
        _check(L.load().expv_mi_memcpy_d2h(self.ctx._h, out.ctypes.data, self.ptr, self.nbytes), self.ctx._h)
        return out

    @property
    def ndim(self):
        return len(self.shape)


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _is_scalar(c):
    """a Python or numpy number (not a bool): what multiplies an operator"""
    return isinstance(c, (int, float, complex, np.number)) and not isinstance(c, (bool, np.bool_))


def _np_dtype_of(x):
    if isinstance(x, DeviceArray):
        return x.dtype
    if _is_torch(x):
        import torch
        return {torch.float64: np.dtype(np.float64), torch.complex128: np.dtype(np.complex128),
                torch.float32: np.dtype(np.float32), torch.complex64: np.dtype(np.complex64)}.get(
            x.dtype, np.dtype(np.float64) if not x.is_complex() else np.dtype(np.complex128))
    return np.asarray(x).dtype


def _code(dt):
    dt = np.dtype(dt)
    if dt.kind == "c":
        return L.C32 if dt.itemsize == 8 else L.C64
    return L.F32 if (dt.kind == "f" and dt.itemsize == 4) else L.F64


_TORCH_NAMES = {"float64": "float64", "complex128": "complex128", "float32": "float32", "complex64": "complex64"}


def _torch_dtype(dt):
    import torch
    return getattr(torch, _TORCH_NAMES[np.dtype(dt).name])


def _ref_dtype(*dts):
    """promote_type of the reference for the given operand element types, restricted to the BlasFloats: Float32 operands give a
    Float32 result there.  The device path computes in fp64 / complex-fp64 (the operands are promoted on upload) and the
    front ends round the result to this type."""
    dt = np.result_type(*[np.dtype(d) for d in dts])
    if dt.kind == "c":
        return np.dtype(np.complex64 if dt.itemsize <= 8 else np.complex128)
    return np.dtype(np.float32 if (dt.kind == "f" and dt.itemsize <= 4) else np.float64)


def _t_dtype(t):
    """element type `t` contributes to promote_type(typeof(t), eltype(A), eltype(b)) (krylov_phiv.jl:142): a numpy scalar keeps
    its own type (np.float64(1.0) with Float32 operands gives Float64, like a Julia Float64), a bare Python float / int /
    complex is a literal and takes the operands' precision."""
    if isinstance(t, np.generic):
        return np.dtype(t.dtype) if t.dtype.kind in "fc" else np.dtype(np.float32)
    # (any Python complex is a Complex in the reference's promote_type, whatever its imaginary part: expv(1 + 0im, A, b) is a
    #  complex vector there -- consistent with _t_parts, which routes every complex t through the complex evaluation)
    return np.dtype(np.complex64) if isinstance(t, complex) else np.dtype(np.float32)


def _src_dtype(A):
    """element type of an operator argument as the caller holds it (MIOperator remembers what it was built from)"""
    if isinstance(A, MIOperator):
        return np.dtype(A.src_dtype)
    if hasattr(A, "indptr") or hasattr(A, "tocsr") or isinstance(A, np.ndarray):      # (any scipy sparse format)
        return np.dtype(A.dtype)
    return _np_dtype_of(A)


def _round_to(x, dtype):
    """a computed result in the reference's result type promote_type(typeof(t), eltype(A), eltype(b)): rounded when that is
    narrower than the work type, widened when a Float64 t met 32-bit operands"""
    dtype = np.dtype(dtype)
    if _np_dtype_of(x) == dtype or isinstance(x, DeviceArray):
        return x
    if _is_torch(x):
        return x.to(_torch_dtype(dtype))
    return np.asarray(x).astype(dtype)


def _work_dtype(*dts):
    """element type the device computes in for operands of these types: the BlasFloat the reference would promote to
    (ExponentialUtilities.jl:19) -- Float32 / ComplexF32 stay 32-bit (half the HBM traffic), everything else is fp64."""
    dts = [np.dtype(d) for d in dts]
    cplx = any(d.kind == "c" for d in dts)
    is32 = all((d.kind == "f" and d.itemsize == 4) or (d.kind == "c" and d.itemsize == 8) for d in dts)
    if is32:
        return np.dtype(np.complex64 if cplx else np.float32)
    return np.dtype(np.complex128 if cplx else np.float64)


def _work64(*dts):
    """the 64-bit work type (entry points whose reference method is Float64-only: kiops)"""
    return np.dtype(np.complex128 if any(np.dtype(d).kind == "c" for d in dts) else np.float64)


def _complex_of(dt):
    dt = np.dtype(dt)
    return np.dtype(np.complex64) if dt.itemsize <= (8 if dt.kind == "c" else 4) else np.dtype(np.complex128)


def _real_of(dt):
    dt = np.dtype(dt)
    return np.dtype(np.float32) if dt.itemsize <= (8 if dt.kind == "c" else 4) else np.dtype(np.float64)


class _Arg:
    """A caller array resolved to (pointer, loc, leading dimension) + what must stay alive."""

    def __init__(self, x, dtype, writable=False):
        self.src = x
        self.dtype = np.dtype(dtype)
        self.back = None
        if isinstance(x, DeviceArray):
            if x.dtype != self.dtype:
                raise TypeError(f"device array has dtype {x.dtype}, need {self.dtype}")
            self.ptr, self.loc, self.shape = x.ptr, L.DEVICE, x.shape
            self.ld = x.shape[0]
            self.keep = x
        elif _is_torch(x):
            import torch
            want = _torch_dtype(self.dtype)
            if not x.is_cuda:
                raise TypeError("torch tensors must live on the GPU (or pass a numpy array)")
            if x.dtype != want:
                if writable:
                    raise TypeError(f"output tensor must be {want}")
                x = x.to(want)
            if x.dim() == 1:
                if x.stride(0) != 1:
                    if writable:
                        raise TypeError("output vector must be contiguous")
                    x = x.contiguous()
                self.ld = x.shape[0]
            else:
                if x.stride(0) != 1:   # need column-major
                    if writable:
                        raise TypeError("output matrix must be column-major (e.g. torch.empty(k, n).t())")
                    x = x.t().contiguous().t()
                self.ld = x.stride(1) if x.shape[1] > 1 else max(x.shape[0], 1)
            # The library works on its own (non-blocking) stream: whatever torch still has in flight for this tensor -- the
            # kernel that produced it, the conversion / layout copy above -- must be complete before the library touches it.
            # (A device-resident dense operator read its column-major copy while torch was still writing it: opnorm 65 instead
            # of 74 at n = 8192.)  An idle stream costs a few microseconds.
            st = torch.cuda.current_stream(x.device)
            if not st.query():
                st.synchronize()
            self.ptr, self.loc, self.shape, self.keep = x.data_ptr(), L.DEVICE, tuple(x.shape), x
        else:
            a = np.asarray(x)
            if writable:
                if a.dtype != self.dtype or not (a.flags.f_contiguous or a.ndim == 1 and a.flags.c_contiguous):
                    # write into a staging array and copy back (keeps Julia-like in-place semantics)
                    self.back = a
                    a = np.empty(a.shape, dtype=self.dtype, order="F")
            else:
                a = np.asfortranarray(a, dtype=self.dtype)
            self.ptr, self.loc, self.shape, self.keep = a.ctypes.data, L.HOST, a.shape, a
            self.ld = a.shape[0] if a.ndim >= 1 else 1
            self.host = a

    def finish(self):
        if self.back is not None:
            if np.iscomplexobj(self.host) and not np.iscomplexobj(self.back):
                raise TypeError("InexactError: complex result into a real array")
            self.back[...] = self.host


def _empty_like(ref, shape, dtype):
    """Allocate an output next to where `ref` lives (numpy -> numpy, torch -> torch, DeviceArray -> same)."""
    dtype = np.dtype(dtype)
    if isinstance(ref, DeviceArray):
        return DeviceArray(shape, dtype, ref.ctx)
    if _is_torch(ref):
        import torch
        tdt = _torch_dtype(dtype)
        if len(shape) == 1:
            return torch.empty(shape[0], dtype=tdt, device=ref.device)
        return torch.empty((shape[1], shape[0]), dtype=tdt, device=ref.device).t()   # column-major
    return np.empty(shape, dtype=dtype, order="F")


# ---------------------------------------------------------------------------------------------
# operators (the contract of docs/src/interfaces.md:7-36)
# ---------------------------------------------------------------------------------------------
def _is_torch_sparse(A):
    """a torch tensor of any layout but the strided one"""
    if not _is_torch(A) or not hasattr(A, "layout"):
        return False
    import torch
    return A.layout != torch.strided


def _unpack_torch_sparse(A):
    """The parts of a 2-D, square, non-batched ``torch.sparse_csr`` / ``torch.sparse_csc`` tensor, on whatever device it lives:
    ``(fmt, ptr, idx, vals, shape)`` with fmt "csr" (ptr = crow_indices, idx = col_indices) or "csc" (ptr = ccol_indices,
    idx = row_indices), the index tensors int32 or int64 and contiguous, the values float32 / float64 / complex64 / complex128.
    No copy of anything that is contiguous already; nothing moves between devices."""
    import torch
    if A.layout == torch.sparse_csr:
        fmt, ptr, idx = "csr", A.crow_indices(), A.col_indices()
    elif A.layout == torch.sparse_csc:
        fmt, ptr, idx = "csc", A.ccol_indices(), A.row_indices()
    else:
        raise TypeError(f"sparse torch tensors must have layout torch.sparse_csr or torch.sparse_csc, not {A.layout} "
                        "(convert with .to_sparse_csr() / .to_sparse_csc())")
    if A.dim() != 2 or ptr.dim() != 1:
        raise DimensionMismatch("a sparse operator is one 2-D matrix (no batch dimensions)")
    if A.shape[0] != A.shape[1]:
        raise DimensionMismatch("operator must be square")
    vals = A.values()
    if vals.dim() != 1:
        raise DimensionMismatch("a sparse operator has scalar entries (no dense dimensions)")
    if vals.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        raise TypeError(f"sparse operator values must be float32 / float64 / complex64 / complex128, not {vals.dtype}")
    if ptr.dtype != idx.dtype or ptr.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"sparse operator indices must be int32 or int64, not {ptr.dtype} / {idx.dtype}")
    return fmt, ptr.contiguous(), idx.contiguous(), vals.contiguous(), (int(A.shape[0]), int(A.shape[1]))


def _is_torch_coo(A):
    if not _is_torch_sparse(A):
        return False
    import torch
    return A.layout == torch.sparse_coo


def _unpack_torch_coo(A):
    """The parts of a 2-D, square, non-hybrid ``torch.sparse_coo`` tensor, coalesced or not, on whatever device it lives:
    ``(row, col, vals, shape)`` -- the two rows of ``A._indices()`` (the public accessors refuse uncoalesced tensors) and
    ``A._values()``, contiguous, without a copy of anything that is contiguous already; nothing moves between devices."""
    import torch
    if A.layout != torch.sparse_coo:
        raise TypeError(f"not a torch.sparse_coo tensor: {A.layout}")
    if A.dense_dim() != 0:
        raise DimensionMismatch("a sparse operator has scalar entries (no dense dimensions)")
    if A.dim() != 2 or A.sparse_dim() != 2:
        raise DimensionMismatch("a sparse operator is one 2-D matrix (no batch dimensions)")
    if A.shape[0] != A.shape[1]:
        raise DimensionMismatch("operator must be square")
    ind, vals = A._indices(), A._values()
    if vals.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        raise TypeError(f"sparse operator values must be float32 / float64 / complex64 / complex128, not {vals.dtype}")
    return ind[0].contiguous(), ind[1].contiguous(), vals.contiguous(), (int(A.shape[0]), int(A.shape[1]))


def _coo_index_arrays(row, col):
    """the two index arrays of a triplet list as the library takes them: both int32 or both int64, contiguous, 1-D, where they lie"""
    if _is_torch(row) != _is_torch(col):
        raise TypeError("from_coo: row and col must both be torch tensors or both be arrays")
    if _is_torch(row):
        import torch
        if row.device != col.device:
            raise ValueError("from_coo: row and col live on different devices")
        if row.dtype != col.dtype or row.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"sparse operator indices must be int32 or int64, not {row.dtype} / {col.dtype}")
        row, col = row.contiguous(), col.contiguous()
        if not row.is_cuda:
            row, col = row.numpy(), col.numpy()
    else:
        row, col = np.asarray(row), np.asarray(col)
        if row.dtype != col.dtype or row.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError(f"sparse operator indices must be int32 or int64, not {row.dtype} / {col.dtype}")
        row, col = np.ascontiguousarray(row), np.ascontiguousarray(col)
    if row.ndim != 1 or col.ndim != 1 or row.shape[0] != col.shape[0]:
        raise DimensionMismatch("from_coo: row and col must be vectors of one length")
    return row, col


def _is_torch_bsr(A):
    if not _is_torch_sparse(A):
        return False
    import torch
    return A.layout in (torch.sparse_bsr, torch.sparse_bsc)


def _unpack_torch_bsr(A):
    """The parts of a 2-D, square, non-batched ``torch.sparse_bsr`` / ``torch.sparse_bsc`` tensor with square blocks, on whatever
    device it lives: ``(compressed, ptr, idx, vals, shape, bd)`` with compressed "rows" (ptr = crow_indices, idx = col_indices) or
    "cols" (ptr = ccol_indices, idx = row_indices), the index tensors int32 or int64 and contiguous, the values ``(nnzb, bd, bd)``
    contiguous -- torch stores row-major blocks in both layouts.  No copy of anything that is contiguous already; nothing moves
    between devices."""
    import torch
    if A.layout == torch.sparse_bsr:
        compressed, ptr, idx = "rows", A.crow_indices(), A.col_indices()
    elif A.layout == torch.sparse_bsc:
        compressed, ptr, idx = "cols", A.ccol_indices(), A.row_indices()
    else:
        raise TypeError(f"block-sparse torch tensors must have layout torch.sparse_bsr or torch.sparse_bsc, not {A.layout}")
    if A.dim() != 2 or ptr.dim() != 1:
        raise DimensionMismatch("a sparse operator is one 2-D matrix (no batch dimensions)")
    if A.shape[0] != A.shape[1]:
        raise DimensionMismatch("operator must be square")
    vals = A.values()
    if vals.dim() != 3:
        raise DimensionMismatch("a sparse operator has scalar entries (no dense dimensions)")
    if vals.shape[1] != vals.shape[2]:
        raise DimensionMismatch(f"a block-sparse operator has square blocks, not {int(vals.shape[1])} x {int(vals.shape[2])} "
                                "(convert with .to_sparse_csr())")
    if vals.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        raise TypeError(f"sparse operator values must be float32 / float64 / complex64 / complex128, not {vals.dtype}")
    if ptr.dtype != idx.dtype or ptr.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"sparse operator indices must be int32 or int64, not {ptr.dtype} / {idx.dtype}")
    return compressed, ptr.contiguous(), idx.contiguous(), vals.contiguous(), (int(A.shape[0]), int(A.shape[1])), int(vals.shape[1])


def _bsr_index_arrays(ptr, idx):
    """the two index arrays of a block-compressed matrix as the library takes them: both int32 or both int64, contiguous, 1-D,
    where they lie (tensors on the GPU stay tensors, anything else becomes a numpy array)"""
    if _is_torch(ptr) != _is_torch(idx):
        raise TypeError("from_bsr: ptr and idx must both be torch tensors or both be arrays")
    if _is_torch(ptr):
        import torch
        if ptr.device != idx.device:
            raise ValueError("from_bsr: ptr and idx live on different devices")
        if ptr.dtype != idx.dtype or ptr.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"sparse operator indices must be int32 or int64, not {ptr.dtype} / {idx.dtype}")
        ptr, idx = ptr.contiguous(), idx.contiguous()
        if not ptr.is_cuda:
            ptr, idx = ptr.numpy(), idx.numpy()
    else:
        ptr, idx = np.asarray(ptr), np.asarray(idx)
        if ptr.dtype != idx.dtype or ptr.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError(f"sparse operator indices must be int32 or int64, not {ptr.dtype} / {idx.dtype}")
        ptr, idx = np.ascontiguousarray(ptr), np.ascontiguousarray(idx)
    if ptr.ndim != 1 or idx.ndim != 1 or ptr.shape[0] < 1:
        raise DimensionMismatch("from_bsr: ptr and idx must be vectors, ptr of one entry per block row (column) plus one")
    return ptr, idx


def _same_index_array(a, b):
    """two index arrays, each a GPU tensor or a numpy array, hold the same integers"""
    if _is_torch(a) and _is_torch(b) and a.device == b.device:
        import torch
        return a.shape == b.shape and bool(torch.equal(a.to(torch.int64), b.to(torch.int64)))
    a, b = (x.cpu().numpy() if _is_torch(x) else np.asarray(x) for x in (a, b))
    return np.array_equal(a, b)


_DIA_ALIGN = {"col": L.DIA_ALIGN_COL, "row": L.DIA_ALIGN_ROW, "start": L.DIA_ALIGN_START}


def _is_scipy_dia(A):
    return hasattr(A, "offsets") and hasattr(A, "data") and getattr(A, "format", None) == "dia"


def _dia_from_scipy(A):
    """``(data, offsets, n)`` of a square scipy ``dia_matrix`` / ``dia_array``, column-aligned as scipy stores it.  scipy allows
    ``data.shape[1] < n``: the missing slots are absent entries, and the rows are padded with zeros here so that every in-matrix
    position of a stored diagonal exists -- the same matrix."""
    if A.shape[0] != A.shape[1]:
        raise DimensionMismatch("operator must be square")
    n = int(A.shape[0])
    data, offsets = np.asarray(A.data), np.asarray(A.offsets, dtype=np.int64)
    if data.shape[1] < n:
        wide = np.zeros((data.shape[0], n), dtype=data.dtype)
        wide[:, :data.shape[1]] = data
        data = wide
    return data, offsets, n


def _dia_layout(data, dt):
    """A 2-D ``data`` array of stored diagonals as the library takes it: ``(keep, ptr, ld, loc)``.  A torch tensor on the GPU stays
    where it is, a CPU tensor or anything else is a numpy array on the host; the element type becomes ``dt``.  Rows must have unit
    stride (``stride(1) == 1``); ``stride(0)`` is handed over as ld, so a view into a wider buffer is taken without a copy."""
    if _is_torch(data) and not data.is_cuda:
        data = data.detach().numpy()
    if _is_torch(data):
        if data.dim() != 2:
            raise DimensionMismatch("from_dia: data must be 2-D, one row per stored diagonal")
        if data.dtype != _torch_dtype(dt):
            data = data.to(_torch_dtype(dt))      # (on the device)
        rows, cols, s0, s1 = int(data.shape[0]), int(data.shape[1]), int(data.stride(0)), int(data.stride(1))
        ptr, loc = data.data_ptr(), L.DEVICE
    else:
        data = np.asarray(data)
        if data.ndim != 2:
            raise DimensionMismatch("from_dia: data must be 2-D, one row per stored diagonal")
        if data.dtype != dt:
            data = data.astype(dt)
        isz = data.dtype.itemsize
        if data.strides[0] % isz or data.strides[1] % isz:
            raise ValueError("from_dia: the strides of data must be whole elements")
        rows, cols, s0, s1 = int(data.shape[0]), int(data.shape[1]), data.strides[0] // isz, data.strides[1] // isz
        ptr, loc = data.ctypes.data, L.HOST
    if rows == 0 or cols == 0:      # nothing stored: the strides of an empty array say nothing
        return data, None, max(cols, 1), loc
    if cols > 1 and s1 != 1:
        raise ValueError(f"from_dia: the rows of data must have unit stride (stride(1) == 1), not {s1}: pass data.contiguous() "
                         "or the transpose's copy")
    if rows > 1 and s0 < cols:
        raise ValueError(f"from_dia: stride(0) = {s0} of data is smaller than its row length {cols} (overlapping or reversed rows)")
    return data, ptr, (s0 if rows > 1 else max(cols, 1)), loc


def _torch_sparse_to_scipy(A):
    """a CPU torch.sparse_csr / sparse_csc tensor as the scipy matrix of the same format (shares the arrays)"""
    import scipy.sparse as sp
    fmt, ptr, idx, vals, shape = _unpack_torch_sparse(A)
    parts = (vals.numpy(), idx.numpy(), ptr.numpy())
    return sp.csr_matrix(parts, shape=shape) if fmt == "csr" else sp.csc_matrix(parts, shape=shape)


def _torch_ready(*tensors):
    """the library works on its own stream: what torch has in flight for these tensors must be complete first (see _Arg)"""
    import torch
    st = torch.cuda.current_stream(tensors[0].device)
    if not st.query():
        st.synchronize()


class MIOperator:
    """Device-resident operator: scipy CSC/CSR matrix, ``torch.sparse_csr`` / ``torch.sparse_csc`` tensor, dense ndarray or
    tensor, or a matrix-free callable; coordinate triplets through ``from_coo``.

    ``MIOperator(A)`` uploads once (CSC is converted to CSR32 on the way; setup cost).  A sparse tensor that lives on the GPU is
    taken where it is (expv_mi_op_create_csr_loc / _csc_loc): its index arrays are checked on the device, only the pattern visits
    the host (``ingest_info``), the values never do.  Coordinate triplets are handed over by name:
    ``MIOperator.from_coo(A)`` for a ``torch.sparse_coo`` tensor (coalesced or not, on either side; ``expv(t, A, b)`` and the
    other front ends take such a tensor as ``A`` directly) and ``MIOperator.from_coo(row, col, vals, n)`` for arrays; repeated
    coordinates are added in entry order (expv_mi_op_create_coo_loc).  ``MIOperator(A)`` itself keeps refusing the layout.  A scipy ``coo_matrix`` keeps going through ``.tocsr()``, whose sum has scipy's order --
    ``from_coo`` is the way to the entry-order sum.  Block-compressed matrices with square blocks (``torch.sparse_bsr`` /
    ``sparse_bsc`` tensors, scipy's ``bsr_matrix``, or the three arrays) come in through ``MIOperator.from_bsr``
    (expv_mi_op_create_bsr_loc) and the front ends take such a tensor as ``A`` too; a scipy ``bsr_matrix`` handed to the plain
    constructor or front ends keeps going through ``.tocsc()``.  Stored diagonals (a scipy ``dia_matrix``, or a 2-D tensor / array
    with one row per diagonal and the offsets) come in through ``MIOperator.from_dia`` (expv_mi_op_create_dia_loc); the plain
    constructor treats a scipy ``dia_matrix`` as before.  ``A.adjoint()`` / ``A.transpose()`` (``A.H`` / ``A.T``) build the operator
    of ``A'`` / ``transpose(A)`` on the device from what ``A`` stores (expv_mi_op_create_adjoint): ``expv(t, A.H, b)``.  ``A + B``, ``A - B``, ``-A``, ``c * A``, ``A / c`` and
    ``MIOperator.lincomb(terms, coefs, identity=None)`` build linear combinations there too (expv_mi_op_create_lincomb), and
    ``C.recombine(coefs)`` changes the coefficients of one: ``expv(t, H0 + f * H1, b)``.  Exposes
    ``shape``, ``dtype``, ``ishermitian`` (LinearAlgebra.ishermitian), ``nnz`` and ``opnorm_inf``.
    """

    def __init__(self, A, ctx=None, dtype=None, ishermitian=None, matvec=None, shape=None, matvec_c=None, _coo=None, _bsr=None, _dia=None):
        lib = L.load()
        self.ctx = ctx or default_context()
        if _is_torch_coo(A):                           # triplets are handed over by name: the constructor stays with compressed layouts
            raise TypeError("MIOperator(A) takes sparse torch tensors of layout torch.sparse_csr or torch.sparse_csc; a "
                            f"{A.layout} tensor holds coordinate triplets: MIOperator.from_coo(A), or pass it to expv / phiv / ... as A")
        if _is_torch_bsr(A):                           # ... and so are blocks
            raise TypeError("MIOperator(A) takes sparse torch tensors of layout torch.sparse_csr or torch.sparse_csc; a "
                            f"{A.layout} tensor holds blocks: MIOperator.from_bsr(A), or pass it to expv / phiv / ... as A")
        if _is_torch_sparse(A) and not A.is_cuda:      # a host matrix in torch's clothes: the scipy path
            A = _torch_sparse_to_scipy(A)
        self.src = A
        h = C.c_void_p()
        self._cb = None
        if _coo is not None:
            dt = self._create_coo(lib, h, *_coo, dtype=dtype)
        elif _bsr is not None:
            dt = self._create_bsr(lib, h, *_bsr, dtype=dtype)
        elif _dia is not None:
            dt = self._create_dia(lib, h, *_dia, dtype=dtype)
        elif matvec_c is not None:       # matrix-free, compiled: (function pointer of type expv_mi_matvec_fn, user pointer) -- what a Julia
            fn, user = matvec_c         # host passes as a @cfunction; nothing of Python runs inside the factorisation
            n = int(shape[0])
            dt = np.dtype(dtype or np.float64)
            self._matvec = None
            self._cb = (fn, user)       # (keeps the caller's objects alive)
            _check(lib.expv_mi_op_create_callback(self.ctx._h, _code(dt), n, C.cast(fn, L.MATVEC_FN),
                                                  C.cast(user, C.c_void_p) if not isinstance(user, (int, type(None))) else C.c_void_p(user),
                                                  int(bool(ishermitian)), 0, C.byref(h)), self.ctx._h)
        elif matvec is not None:        # matrix-free: matvec(x_dev_tensor) -> y_dev_tensor (torch, on the stream)
            n = int(shape[0])
            dt = np.dtype(dtype or np.float64)
            self._matvec = matvec

            def _cb(user, xp, yp, stream):
                try:
                    import torch
                    x = _torch_view(xp, n, dt)
                    y = _torch_view(yp, n, dt)
                    with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                        y.copy_(matvec(x))
                    return 0
                except Exception:   # pragma: no cover - surfaced as ArgumentError by the library
                    import traceback
                    traceback.print_exc()
                    return 1

            self._cb = L.MATVEC_FN(_cb)
            _check(lib.expv_mi_op_create_callback(self.ctx._h, _code(dt), n, self._cb, None,
                                                  int(bool(ishermitian)), 0, C.byref(h)), self.ctx._h)
        elif _is_torch_sparse(A):       # CSR / CSC arrays that live on the device: no host copy made here
            fmt, ptr, idx, vals, shp = _unpack_torch_sparse(A)
            if A.device.index not in (None, self.ctx.device):
                raise ValueError(f"sparse tensor lives on {A.device}, the context on device {self.ctx.device}")
            dt = _work_dtype(_np_dtype_of(vals) if dtype is None else dtype)
            if vals.dtype != _torch_dtype(dt):
                vals = vals.to(_torch_dtype(dt))      # (on the device)
            _torch_ready(ptr, idx, vals)
            self._sp_format, self._sp_sorted = fmt, True
            self._dev_parts = (ptr, idx)              # pattern of the caller's arrays: update_values compares, astype rebuilds
            create = lib.expv_mi_op_create_csr_loc if fmt == "csr" else lib.expv_mi_op_create_csc_loc
            _check(create(self.ctx._h, _code(dt), shp[0], int(idx.numel()), ptr.data_ptr(), idx.data_ptr(), vals.data_ptr(),
                          ptr.element_size(), 0, L.DEVICE, C.byref(h)), self.ctx._h)
        elif hasattr(A, "tocsc") and (hasattr(A, "indptr") or hasattr(A, "tocsr")):
            if not hasattr(A, "indptr"):
                A = A.tocsr()
            dt = _work_dtype(A.dtype if dtype is None else dtype)
            n = A.shape[0]
            if A.shape[0] != A.shape[1]:
                raise DimensionMismatch("operator must be square")
            self._sp_format = "csr" if A.format == "csr" else "csc"
            self._sp_sorted = bool(A.has_sorted_indices) if A.format in ("csr", "csc") else False
            if A.format == "csr":
                M = A.astype(dt)
                M.sort_indices()
                ip, ix = M.indptr, M.indices
                ib = 8 if ip.dtype.itemsize == 8 else 4
                ip = np.ascontiguousarray(ip, dtype=np.int64 if ib == 8 else np.int32)
                ix = np.ascontiguousarray(ix, dtype=np.int64 if ib == 8 else np.int32)
                vals = np.ascontiguousarray(M.data, dtype=dt)
                _check(lib.expv_mi_op_create_csr(self.ctx._h, _code(dt), n, ip.ctypes.data, ix.ctypes.data,
                                                 vals.ctypes.data, ib, 0, C.byref(h)), self.ctx._h)
            else:                       # Julia's SparseMatrixCSC layout
                M = A.tocsc().astype(dt)
                M.sort_indices()
                cp = np.ascontiguousarray(M.indptr, dtype=np.int64)
                rv = np.ascontiguousarray(M.indices, dtype=np.int64)
                vals = np.ascontiguousarray(M.data, dtype=dt)
                _check(lib.expv_mi_op_create_csc(self.ctx._h, _code(dt), n, cp.ctypes.data, rv.ctypes.data,
                                                 vals.ctypes.data, 0, C.byref(h)), self.ctx._h)
        else:
            if _is_torch(A):
                dt = _np_dtype_of(A)
                arg = _Arg(A, dt)
                n = A.shape[0]
                _check(lib.expv_mi_op_create_dense(self.ctx._h, _code(dt), n, arg.ptr, arg.ld, L.DEVICE,
                                                   C.byref(h)), self.ctx._h)
                self._keep = arg
            else:
                M = np.asarray(A)
                dt = _work_dtype(M.dtype if dtype is None else dtype)
                if M.ndim != 2 or M.shape[0] != M.shape[1]:
                    raise DimensionMismatch("operator must be square")
                n = M.shape[0]
                arg = None
                if n >= 256 and not M.flags.f_contiguous:
                    # a row-major array would be transposed on the host first (numpy: 4 s at n = 8192): upload it as it lies
                    # and lay it out column-major on the device (torch is the device-memory plumbing here).  torch is optional:
                    # without a usable ROCm build the host transpose below does the same job, slower.
                    try:
                        import torch
                        Ad = torch.as_tensor(np.ascontiguousarray(M, dtype=dt), device="cuda:%d" % self.ctx.device)
                        arg = _Arg(Ad, dt)
                        del Ad
                    except (ImportError, RuntimeError, AssertionError):
                        arg = None
                if arg is not None:
                    _check(lib.expv_mi_op_create_dense(self.ctx._h, _code(dt), n, arg.ptr, arg.ld, L.DEVICE,
                                                       C.byref(h)), self.ctx._h)
                    self._keep = arg
                else:
                    M = np.asfortranarray(M, dtype=dt)
                    _check(lib.expv_mi_op_create_dense(self.ctx._h, _code(dt), n, M.ctypes.data, max(n, 1), L.HOST,
                                                       C.byref(h)), self.ctx._h)
        self._h = h
        self._finalizer = weakref.finalize(self, lib.expv_mi_op_destroy, h)
        try:            # element type the caller handed over (Float32 operands: see _ref_dtype)
            if _coo is not None:
                self.src_dtype = _np_dtype_of(_coo[2]) if _is_torch(_coo[2]) else np.dtype(np.asarray(_coo[2]).dtype)
            elif _bsr is not None:
                self.src_dtype = _np_dtype_of(_bsr[2]) if _is_torch(_bsr[2]) else np.dtype(np.asarray(_bsr[2]).dtype)
            elif _dia is not None:
                self.src_dtype = _np_dtype_of(_dia[0]) if _is_torch(_dia[0]) else np.dtype(np.asarray(_dia[0]).dtype)
            elif A is None:
                self.src_dtype = np.dtype(dtype or np.float64)
            elif hasattr(A, "indptr") or isinstance(A, np.ndarray):
                self.src_dtype = np.dtype(A.dtype)
            elif _is_torch_sparse(A):
                self.src_dtype = _np_dtype_of(A.values())
            else:
                self.src_dtype = _np_dtype_of(A)
        except Exception:
            self.src_dtype = np.dtype(np.float64)
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        _check(lib.expv_mi_op_info(h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)))
        self.shape = (int(n_.value), int(n_.value))
        self.nnz = int(nnz.value)
        self.ishermitian = bool(herm.value) if ishermitian is None else bool(ishermitian)
        self.opnorm_inf = float(opn.value)
        self.dtype = np.dtype({L.F64: np.float64, L.C64: np.complex128, L.F32: np.float32, L.C32: np.complex64}[dtc.value])

    @classmethod
    def from_coo(cls, row, col=None, vals=None, n=None, index_base=0, ctx=None, dtype=None):
        """``from_coo(A)``: the operator of a 2-D, square ``torch.sparse_coo`` tensor, coalesced or not, on the GPU or the CPU
        (read through ``A._indices()`` / ``A._values()``, no copy of what is contiguous).  ``from_coo(row, col, vals, n)``:
        the n x n operator of the coordinate triplets ``(row[k], col[k], vals[k])`` (expv_mi_op_create_coo_loc): numpy arrays
        or torch tensors, indices int32 or int64 with the given base, in any order, repeats allowed.  Entries of one coordinate
        are ADDED, in the operator's element type and in ascending order of k -- Julia's ``sparse(I, J, V, n, n)``, with the
        order of the sum fixed -- and a sum that comes out as zero stays stored.  Tensors on the GPU are taken where they are
        (checked, sorted and compressed on the device; the values never visit the host); host arrays are staged and take the same
        path, so both give the same bits.  ``update_values`` then takes one value per triplet, in triplet order."""
        if _is_torch_coo(row):
            if col is not None or vals is not None:
                raise TypeError("from_coo: either one torch.sparse_coo tensor or row, col, vals, n")
            row, col, vals, shp = _unpack_torch_coo(row)
            if n is not None and int(n) != shp[0]:
                raise DimensionMismatch("from_coo: n differs from the tensor's shape")
            n, index_base = shp[0], 0
        elif col is None or vals is None or n is None:
            raise TypeError("from_coo: row, col, vals and n are required")
        return cls(None, ctx, dtype=dtype, _coo=(row, col, vals, int(n), int(index_base)))

    def _create_coo(self, lib, h, row, col, vals, n, index_base, dtype=None):
        row, col = _coo_index_arrays(row, col)
        on_dev = _is_torch(row)
        dt = _work_dtype((_np_dtype_of(vals) if _is_torch(vals) else np.asarray(vals).dtype) if dtype is None else dtype)
        if on_dev:
            import torch
            if row.device.index not in (None, self.ctx.device):
                raise ValueError(f"triplets live on {row.device}, the context on device {self.ctx.device}")
            vals = torch.as_tensor(vals, device=row.device)
            if vals.dtype != _torch_dtype(dt):
                vals = vals.to(_torch_dtype(dt))      # (on the device)
            vals = vals.contiguous()
            _torch_ready(row, col, vals)
            ptrs, nent = (row.data_ptr(), col.data_ptr(), vals.data_ptr()), int(row.numel())
            isz, nval, loc = row.element_size(), int(vals.numel()), L.DEVICE
        else:
            if _is_torch(vals):
                vals = vals.cpu().numpy()
            vals = np.ascontiguousarray(vals, dtype=dt)
            ptrs, nent = (row.ctypes.data, col.ctypes.data, vals.ctypes.data), int(row.shape[0])
            isz, nval, loc = row.dtype.itemsize, int(vals.size), L.HOST
        if vals.ndim != 1 or nval != nent:
            raise DimensionMismatch("from_coo: one value per (row, col) pair expected")
        self._sp_format, self._sp_sorted = "coo", True
        self._coo_parts = (row, col, vals, int(n), int(index_base))      # update_values compares, astype rebuilds
        _check(lib.expv_mi_op_create_coo_loc(self.ctx._h, _code(dt), int(n), nent, ptrs[0] if nent else None, ptrs[1] if nent else None,
                                             ptrs[2] if nent else None, isz, int(index_base), loc, C.byref(h)), self.ctx._h)
        return dt

    @classmethod
    def from_bsr(cls, ptr, idx=None, vals=None, n=None, index_base=0, compressed="rows", block_order="row", ctx=None, dtype=None):
        """``from_bsr(A)``: the operator of a 2-D, square ``torch.sparse_bsr`` / ``torch.sparse_bsc`` tensor with square blocks, on
        the GPU or the CPU, or of a scipy ``bsr_matrix`` with square blocks.  ``from_bsr(ptr, idx, vals)``: the operator of the
        block-compressed arrays (expv_mi_op_create_bsr_loc), numpy arrays or torch tensors: ``ptr`` over the block rows
        (``compressed="rows"``, BSR) or block columns (``"cols"``, BSC), ``idx`` the block columns (rows), int32 or int64 with the
        given base, ``vals`` of shape ``(nnzb, bd, bd)`` holding each block row-major (``block_order="row"``: torch, scipy) or
        column-major (``"col"``); ``n`` defaults to ``(len(ptr) - 1) * bd``.  The operator is the scalar matrix of scipy's
        ``bsr_matrix((vals, idx, ptr)).tocsr()``: every element of a stored block is a stored entry, zeros included.  Tensors on
        the GPU are taken where they are (checked and expanded on the device; the values never visit the host unless a block row
        is unsorted); host data is staged and takes the same path, so both give the same bits.  ``update_values`` then takes the
        values in the same block order."""
        if _is_torch_bsr(ptr) or (hasattr(ptr, "indptr") and getattr(ptr, "format", None) == "bsr"):
            if idx is not None or vals is not None:
                raise TypeError("from_bsr: either one block-sparse matrix or ptr, idx, vals")
            if _is_torch_bsr(ptr):
                compressed, ptr, idx, vals, shp, _ = _unpack_torch_bsr(ptr)
            else:
                A = ptr
                if A.shape[0] != A.shape[1]:
                    raise DimensionMismatch("operator must be square")
                if A.blocksize[0] != A.blocksize[1]:
                    raise DimensionMismatch(f"a block-sparse operator has square blocks, not {A.blocksize[0]} x {A.blocksize[1]} "
                                            "(convert with .tocsr())")
                compressed, ptr, idx, vals, shp = "rows", A.indptr, A.indices, A.data, tuple(int(x) for x in A.shape)
            if n is not None and int(n) != shp[0]:
                raise DimensionMismatch("from_bsr: n differs from the matrix's shape")
            n, index_base, block_order = shp[0], 0, "row"
        elif idx is None or vals is None:
            raise TypeError("from_bsr: ptr, idx and vals are required")
        if compressed not in ("rows", "cols") or block_order not in ("row", "col"):
            raise ValueError('from_bsr: compressed is "rows" or "cols", block_order "row" or "col"')
        return cls(None, ctx, dtype=dtype, _bsr=(ptr, idx, vals, n, int(index_base), compressed, block_order))

    def _create_bsr(self, lib, h, ptr, idx, vals, n, index_base, compressed, block_order, dtype=None):
        ptr, idx = _bsr_index_arrays(ptr, idx)
        on_dev = _is_torch(ptr)
        dt = _work_dtype((_np_dtype_of(vals) if _is_torch(vals) else np.asarray(vals).dtype) if dtype is None else dtype)
        if on_dev:
            import torch
            if ptr.device.index not in (None, self.ctx.device):
                raise ValueError(f"block arrays live on {ptr.device}, the context on device {self.ctx.device}")
            vals = torch.as_tensor(vals, device=ptr.device)
            if vals.dtype != _torch_dtype(dt):
                vals = vals.to(_torch_dtype(dt))      # (on the device)
            vals = vals.contiguous()
            _torch_ready(ptr, idx, vals)
            ptrs, nnzb, isz, loc = (ptr.data_ptr(), idx.data_ptr(), vals.data_ptr()), int(idx.numel()), ptr.element_size(), L.DEVICE
        else:
            if _is_torch(vals):
                vals = vals.cpu().numpy()
            vals = np.ascontiguousarray(vals, dtype=dt)
            ptrs, nnzb, isz, loc = (ptr.ctypes.data, idx.ctypes.data, vals.ctypes.data), int(idx.shape[0]), ptr.dtype.itemsize, L.HOST
        if vals.ndim != 3 or int(vals.shape[0]) != nnzb or vals.shape[1] != vals.shape[2] or int(vals.shape[1]) < 1:
            raise DimensionMismatch("from_bsr: vals of shape (nnzb, bd, bd) expected, one square block per block index")
        bd = int(vals.shape[1])
        n = (int(ptr.shape[0]) - 1) * bd if n is None else int(n)
        if n != (int(ptr.shape[0]) - 1) * bd:
            raise DimensionMismatch("from_bsr: ptr must have n / bd + 1 entries")
        layout = (L.BSR_BLOCK_COL_MAJOR if block_order == "col" else L.BSR_BLOCK_ROW_MAJOR) | (L.BSR_COMPRESSED_COLS if compressed == "cols" else 0)
        self._sp_format, self._sp_sorted = "bsr", True
        self._bsr_parts = (ptr, idx, vals, n, int(index_base), compressed, block_order)      # update_values compares, astype rebuilds
        _check(lib.expv_mi_op_create_bsr_loc(self.ctx._h, _code(dt), n, nnzb, bd, ptrs[0], ptrs[1] if nnzb else None,
                                             ptrs[2] if nnzb else None, isz, int(index_base), layout, loc, C.byref(h)), self.ctx._h)
        return dt

    @classmethod
    def from_dia(cls, data, offsets=None, n=None, align="col", ctx=None, dtype=None):
        """``from_dia(A)``: the operator of a square scipy ``dia_matrix`` / ``dia_array``.  ``from_dia(data, offsets, n)``: the
        n x n operator of stored diagonals (expv_mi_op_create_dia_loc): ``offsets`` the diagonals' offsets k = column - row in any
        order, ``data`` a 2-D torch tensor (GPU or CPU) or numpy array with one row per offset and unit stride along the rows
        (``stride(0)`` may be larger than the row length: it is handed over as ld).  ``align`` says where element (i, i + k) lies
        in its row: ``"col"`` at column i + k (scipy, LAPACK band rows), ``"row"`` at column i (the DIA of GPU sparse libraries),
        ``"start"`` at column min(i, i + k) (compact vectors).  ``n`` defaults to the row length (``"start"``: plus the smallest
        |k|).  The pattern is decided by the offsets alone: every in-matrix position of a stored diagonal is a stored entry,
        zeros included -- scipy's ``.tocsr()`` without its dropping of zeros; slots that correspond to no matrix position are
        never read.  A tensor on the GPU is expanded where it is; host data is staged and takes the same path.
        ``update_values`` then takes a ``data`` array of the same shape, strides and alignment."""
        if _is_scipy_dia(data):
            if offsets is not None:
                raise TypeError("from_dia: either one scipy dia matrix or data, offsets")
            data, offsets, n2 = _dia_from_scipy(data)
            if n is not None and int(n) != n2:
                raise DimensionMismatch("from_dia: n differs from the matrix's shape")
            n, align = n2, "col"
        elif offsets is None:
            raise TypeError("from_dia: data and offsets are required")
        if align not in _DIA_ALIGN:
            raise ValueError('from_dia: align is "col", "row" or "start"')
        return cls(None, ctx, dtype=dtype, _dia=(data, offsets, n, align))

    def _create_dia(self, lib, h, data, offsets, n, align, dtype=None):
        offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if _is_torch(offsets) else offsets), dtype=np.int64)
        dt = _work_dtype((_np_dtype_of(data) if _is_torch(data) else np.asarray(data).dtype) if dtype is None else dtype)
        data, ptr, ld, loc = _dia_layout(data, dt)
        if offsets.ndim != 1 or int(data.shape[0]) != offsets.shape[0]:
            raise DimensionMismatch("from_dia: one row of data per offset expected")
        if loc == L.DEVICE:
            if data.device.index not in (None, self.ctx.device):
                raise ValueError(f"data lives on {data.device}, the context on device {self.ctx.device}")
            _torch_ready(data)
        if n is None:
            n = int(data.shape[1]) + (int(np.abs(offsets).min()) if align == "start" and offsets.size else 0)
        n = int(n)
        self._sp_format, self._sp_sorted = "dia", True
        self._dia_parts = (data, offsets, n, align, ld)      # update_values compares, astype rebuilds
        _check(lib.expv_mi_op_create_dia_loc(self.ctx._h, _code(dt), n, int(offsets.shape[0]), offsets.ctypes.data,
                                             ptr if data.shape[0] and data.shape[1] else None, ld, _DIA_ALIGN[align], loc, C.byref(h)),
               self.ctx._h)
        return dt

    @property
    def reorder_info(self):
        """How the operator is stored (expv_mi_op_reorder_info): ``reordered`` -- as P A P' with P a bandwidth-reducing ordering
        (context option "reorder"; every call permutes vectors on entry and exit, results are those of the natural ordering) --
        and the bandwidth before / after, the ordering's share of the creation time."""
        out = (C.c_int64 * 4)()
        _check(L.load().expv_mi_op_reorder_info(self._h, out))
        return {"reordered": bool(out[0]), "bandwidth_before": int(out[1]), "bandwidth_after": int(out[2]), "setup_s": 1e-6 * int(out[3])}

    @property
    def patch_info(self):
        """Grid-patch storage of a 2-D grid stencil (expv_mi_op_patch_info; context option "patch")."""
        out = (C.c_int64 * 8)()
        _check(L.load().expv_mi_op_patch_info(self._h, out))
        return {"patch_form": bool(out[0]), "grid_row_length": int(out[1]), "tiles": int(out[2]), "longest_ring": int(out[3]),
                "mean_ring": (float(out[4]) / int(out[2])) if out[2] else 0.0, "tiles_ring_over_128": int(out[5]),
                "column_indices_stored": int(out[6]), "ring_entries_per_tile": int(out[7])}

    @property
    def elide_info(self):
        """Constant tiles of a banded Float64 operator (expv_mi_op_elide_info; context option "elide"): ``tiles`` of 512 stored rows,
        ``diagonals``, ``constant_pairs`` -- the (tile, diagonal) pairs on which the stored diagonal holds one bit pattern, which the
        single-pass step reads as one entry instead of streaming --, ``wholly_constant`` -- every diagonal constant on all its rows --
        and ``mask``: one uint8 per tile, bit d = diagonal d.  All zero / empty for operators without that stored form."""
        out = (C.c_int64 * 4)()
        _check(L.load().expv_mi_op_elide_info(self._h, out, None, 0))
        mask = np.zeros(int(out[0]), dtype=np.uint8)
        if mask.size:
            _check(L.load().expv_mi_op_elide_info(self._h, out, mask.ctypes.data, mask.size))
        return {"tiles": int(out[0]), "diagonals": int(out[1]), "constant_pairs": int(out[2]), "wholly_constant": bool(out[3]), "mask": mask}

    @property
    def ingest_info(self):
        """How a sparse operator came to be (expv_mi_op_ingest_info): ``from_device`` -- created from arrays on the device --,
        the bytes of pattern and of values that were brought to the host for it (values: 0 unless a row is unsorted or holds a
        duplicate), the creation time and the share of the device checks, whether the ordering plan came from the plan cache, and
        for an operator made from triplets ``coo_entries`` -- how many were handed over -- and the ``sort_passes`` that ran."""
        out = (C.c_int64 * 8)()
        _check(L.load().expv_mi_op_ingest_info(self._h, out))
        return {"from_device": bool(out[0]), "pattern_bytes_to_host": int(out[1]), "value_bytes_to_host": int(out[2]),
                "create_s": 1e-6 * int(out[3]), "ingest_s": 1e-6 * int(out[4]), "plan_cached": bool(out[5]),
                "coo_entries": int(out[6]), "sort_passes": int(out[7])}

    def update_values(self, A):
        """New values on the same sparsity pattern (expv_mi_op_update_values): ``A`` is the matrix the operator was created
        from after an in-place change of its values (same format, sorted indices; for an operator made from a sparse device
        tensor: a tensor of the same layout, shape and nnz), a device tensor or an array of nnz values in that order.  The stored
        device forms are refilled and ishermitian / opnorm_inf re-evaluated, ~10x cheaper than a new MIOperator."""
        fmt = getattr(self, "_sp_format", None)
        if fmt is None:
            raise ValueError("update_values: sparse operators only")
        if getattr(self, "_adj_how", 0) and (_is_torch_sparse(A) or hasattr(A, "indptr")):
            raise TypeError("update_values: an operator made by adjoint() / transpose() takes bare values in its own sorted-row order; "
                            "to follow its parent use refresh(parent), for another element type parent.astype(dtype).adjoint()")
        if getattr(self, "_lc_terms", None) is not None and (_is_torch_sparse(A) or hasattr(A, "indptr")):
            raise TypeError("update_values: an operator made by lincomb() (or by + - * /) takes bare values in its own sorted-row order; "
                            "to follow its terms or change its coefficients use recombine(coefs)")
        if fmt == "coo":
            return self._update_coo(A)
        if fmt == "bsr":
            return self._update_bsr(A)
        if fmt == "dia":
            return self._update_dia(A)
        if _is_torch_sparse(A):
            if not hasattr(self, "_dev_parts"):
                raise ValueError("update_values: a sparse tensor refreshes an operator that was created from one")
            f2, ptr, idx, vals, shp = _unpack_torch_sparse(A)
            if f2 != fmt or shp != self.shape or int(idx.numel()) != self.nnz or not A.is_cuda:
                raise ValueError("update_values: same layout, shape and nnz as at creation required (on the device)")
            self.src = A
        elif hasattr(A, "indptr"):
            if A.format != fmt or not A.has_sorted_indices or A.nnz != self.nnz or A.shape != self.shape:
                raise ValueError("update_values: same format, shape and (sorted) pattern as at creation required")
            vals = A.data
        else:
            vals = A
        arg = _Arg(vals if _is_torch(vals) else np.ascontiguousarray(vals, dtype=self.dtype), self.dtype)
        if int(np.prod(arg.shape)) != self.nnz:
            raise DimensionMismatch("update_values: nnz values expected")
        _check(L.load().expv_mi_op_update_values(self._h, arg.ptr, arg.loc), self.ctx._h)
        if hasattr(A, "indptr"):
            self.src = A
        elif hasattr(self, "_dev_parts") and not _is_torch_sparse(A):
            # device-born operator refreshed with bare values: what astype rebuilds from is the creation pattern + these values
            import torch
            ptr, idx = self._dev_parts
            v = arg.keep if arg.loc == L.DEVICE else torch.as_tensor(arg.host, device=ptr.device)
            mk = torch.sparse_csr_tensor if fmt == "csr" else torch.sparse_csc_tensor
            self.src = mk(ptr, idx, v.reshape(-1), size=self.shape)
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        _check(L.load().expv_mi_op_info(self._h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)))
        self.ishermitian = bool(herm.value)
        self.opnorm_inf = float(opn.value)
        for key in [k for k in vars(self) if k.startswith("_as_")]:      # converted copies hold the old values
            delattr(self, key)
        return self

    def _update_coo(self, A):
        """update_values of an operator made from triplets: one value per triplet in triplet order (an array, a tensor, or a
        torch.sparse_coo tensor with the indices of the creation); summed as at creation, bit-equal to creating anew"""
        row, col, old, n, base = self._coo_parts
        nent = int(row.shape[0])
        if _is_torch_coo(A):
            r2, c2, vals, shp = _unpack_torch_coo(A)
            same = shp == self.shape and int(r2.shape[0]) == nent and _is_torch(row) == r2.is_cuda
            if same and _is_torch(row):
                import torch
                same = r2.dtype == row.dtype and bool(torch.equal(r2, row)) and bool(torch.equal(c2, col))
            elif same:
                same = np.array_equal(r2.numpy() - 0, row - base) and np.array_equal(c2.numpy() - 0, col - base)
            if not same:
                raise ValueError("update_values: a sparse_coo tensor with the shape and the indices of the creation required")
        else:
            vals = A
        if _is_torch(vals) and not vals.is_cuda:
            vals = vals.numpy()
        arg = _Arg(vals if _is_torch(vals) else np.ascontiguousarray(vals, dtype=self.dtype), self.dtype)
        if len(arg.shape) != 1 or int(arg.shape[0]) != nent:
            raise DimensionMismatch("update_values: one value per triplet of the creation expected (%d)" % nent)
        _check(L.load().expv_mi_op_update_values(self._h, arg.ptr, arg.loc), self.ctx._h)
        self._coo_parts = (row, col, arg.keep, n, base)
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        _check(L.load().expv_mi_op_info(self._h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)))
        self.ishermitian = bool(herm.value)
        self.opnorm_inf = float(opn.value)
        for key in [k for k in vars(self) if k.startswith("_as_")]:      # converted copies hold the old values
            delattr(self, key)
        return self

    def _update_bsr(self, A):
        """update_values of an operator made from block arrays: the values in the block order of the creation -- a
        ``(nnzb, bd, bd)`` or flat array or tensor, or a block-sparse matrix of the layout, shape, block size and indices of the
        creation; permuted as at creation, bit-equal to creating anew"""
        ptr, idx, old, n, base, compressed, order = self._bsr_parts
        nnzb, bd = int(old.shape[0]), int(old.shape[1])
        if _is_torch_bsr(A) or (hasattr(A, "indptr") and getattr(A, "format", None) == "bsr"):
            if _is_torch_bsr(A):
                c2, p2, i2, vals, shp, bd2 = _unpack_torch_bsr(A)
            else:
                c2, p2, i2, vals, shp, bd2 = "rows", A.indptr, A.indices, A.data, tuple(A.shape), (A.blocksize[0] if A.blocksize[0] == A.blocksize[1] else -1)
            same = (c2, tuple(shp), bd2, "row") == (compressed, self.shape, bd, order) and int(i2.shape[0]) == nnzb
            if not (same and _same_index_array(p2 + base, ptr) and _same_index_array(i2 + base, idx)):
                raise ValueError("update_values: a block-sparse matrix with the layout, shape, block size and indices of the creation required")
        else:
            vals = A
        if _is_torch(vals) and not vals.is_cuda:
            vals = vals.numpy()
        vals = vals.contiguous() if _is_torch(vals) else np.ascontiguousarray(vals, dtype=self.dtype)
        if tuple(vals.shape) not in ((nnzb, bd, bd), (nnzb * bd * bd,)):
            raise DimensionMismatch("update_values: the values of the creation's blocks expected, (%d, %d, %d) or flat" % (nnzb, bd, bd))
        arg = _Arg(vals.reshape(-1), self.dtype)
        _check(L.load().expv_mi_op_update_values(self._h, arg.ptr, arg.loc), self.ctx._h)
        self._bsr_parts = (ptr, idx, arg.keep.reshape(nnzb, bd, bd), n, base, compressed, order)
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        _check(L.load().expv_mi_op_info(self._h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)))
        self.ishermitian = bool(herm.value)
        self.opnorm_inf = float(opn.value)
        for key in [k for k in vars(self) if k.startswith("_as_")]:      # converted copies hold the old values
            delattr(self, key)
        return self

    def _update_dia(self, A):
        """update_values of an operator made from stored diagonals: a ``data`` array or tensor of the creation's shape, strides
        and alignment (padding is not read), or a scipy dia matrix of the creation's shape and offsets; transposed as at creation,
        bit-equal to creating anew"""
        old, offsets, n, align, ld = self._dia_parts
        if _is_scipy_dia(A):
            data, off2, n2 = _dia_from_scipy(A)
            if n2 != n or align != "col" or not np.array_equal(off2, offsets):
                raise ValueError("update_values: a dia matrix with the shape and offsets of the creation required")
        else:
            data = A
        data, ptr, ld2, loc = _dia_layout(data, self.dtype)
        if tuple(data.shape) != tuple(old.shape) or ld2 != ld:
            raise DimensionMismatch("update_values: data of the creation's shape %s and row stride %d expected" % (tuple(old.shape), ld))
        if loc == L.DEVICE:
            _torch_ready(data)
        _check(L.load().expv_mi_op_update_values(self._h, ptr if self.nnz else None, loc), self.ctx._h)
        self._dia_parts = (data, offsets, n, align, ld)
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        _check(L.load().expv_mi_op_info(self._h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)))
        self.ishermitian = bool(herm.value)
        self.opnorm_inf = float(opn.value)
        for key in [k for k in vars(self) if k.startswith("_as_")]:      # converted copies hold the old values
            delattr(self, key)
        return self

    def _adjoint(self, how):
        lib = L.load()
        h = C.c_void_p()
        _check(lib.expv_mi_op_create_adjoint(self._h, how, C.byref(h)), self.ctx._h)
        op = object.__new__(MIOperator)
        op.ctx, op.src, op._cb, op._matvec, op._h = self.ctx, None, None, None, h
        op._finalizer = weakref.finalize(op, lib.expv_mi_op_destroy, h)
        op._adj_how = how
        op.src_dtype = self.src_dtype
        if getattr(self, "_sp_format", None) is not None:      # sparse: bare values refresh it in its own sorted-row order
            op._sp_format, op._sp_sorted = "csr", True
        op._read_info()
        return op

    def _read_info(self):
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        _check(L.load().expv_mi_op_info(self._h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)))
        self.shape = (int(n_.value), int(n_.value))
        self.nnz = int(nnz.value)
        self.ishermitian = bool(herm.value)
        self.opnorm_inf = float(opn.value)
        self.dtype = np.dtype({L.F64: np.float64, L.C64: np.complex128, L.F32: np.float32, L.C32: np.complex64}[dtc.value])

    def adjoint(self):
        """The operator of ``A' = conj(transpose(A))`` as a NEW, independent ``MIOperator`` on the same context
        (expv_mi_op_create_adjoint): built on the device from what this operator stores, whatever it was created from -- sparse of
        any birth, reordered or not, or dense (an owned packed copy); the values never visit the host.  ``expv(t, A.adjoint(), b)``
        is the reference's ``expv(t, A', b)``: the adjoint-sensitivity call, the left-eigenvector call.  It does not follow later
        changes of ``A`` (``refresh`` does that) and survives ``A``.  ``shape``, ``dtype``, ``nnz``, ``ishermitian`` and
        ``opnorm_inf`` are filled as for any operator -- ``A.adjoint().opnorm_inf`` is the one-norm of ``A``.  ``src`` is ``None``:
        ``astype`` is refused (``A.astype(dtype).adjoint()``), ``update_values`` takes bare values only, nnz of them in the
        adjoint's own sorted-row order (the column-major order of ``A``).  A matrix-free operator has no adjoint (Unsupported).
        ``A.H`` is an alias and, as in scipy, builds a new operator at every access: keep the result."""
        return self._adjoint(L.OP_ADJOINT)

    def transpose(self):
        """The operator of ``transpose(A)``, no conjugation: see ``adjoint``, with which it shares everything else (for the real
        element types also the bits).  ``A.T`` is an alias that builds a new operator at every access."""
        return self._adjoint(L.OP_TRANSPOSE)

    _NORMEST_INFO = ("iterations", "applications", "host_reads", "index", "resamples", "exit", "temporary_adjoint", "adjoint_us")

    def norm_power(self, p, ord=np.inf, shift=0.0, adjoint=None, return_info=False):
        """A lower bound of ``||(A - shift I)^p||`` in the infinity norm (``ord=inf``) or the 1-norm (``ord=1``), 1 <= p <= 16, by the
        deterministic block 1-norm estimator on the device (expv_mi_op_norm_power; Higham & Tisseur 2000, t = 2): 2 p operator
        applications per column and iteration, at most five iterations, no power is formed.  ``adjoint``: an operator of ``A'``
        (``A.adjoint()``); None: a Hermitian operator serves as its own, otherwise one is made for the call.  p = 1 with ``ord=inf`` is
        the exact row-sum norm.  ``ord`` is ``np.inf`` or the integer 1; anything else is refused.  ``return_info``: also the dictionary kept in ``self.last_norm_info`` (iterations, applications,
        host_reads, index, resamples, exit, temporary_adjoint, adjoint_us)."""
        if isinstance(ord, (bool, np.bool_)):
            which = -1
        elif isinstance(ord, (float, np.floating)) and ord == np.inf:
            which = 0
        elif isinstance(ord, (int, np.integer)) and ord == 1:
            which = 1
        else:
            which = -1      # (anything but inf and 1: refused by the library)
        if adjoint is not None and not isinstance(adjoint, MIOperator):
            raise TypeError("norm_power: adjoint must be an MIOperator (A.adjoint())")
        sh = complex(shift)
        info, est = (C.c_int64 * 8)(), C.c_double(0.0)
        _check(L.load().expv_mi_op_norm_power(self._h, None if adjoint is None else adjoint._h, int(p), sh.real, sh.imag, which, info,
                                              C.byref(est)), self.ctx._h)
        self.last_norm_info = dict(zip(self._NORMEST_INFO, (int(v) for v in info)))
        return (float(est.value), self.last_norm_info) if return_info else float(est.value)

    H = property(adjoint, doc="``adjoint()``: a new operator at every access (the scipy convention), not cached")
    T = property(transpose, doc="``transpose()``: a new operator at every access (the scipy convention), not cached")

    def refresh(self, parent):
        """Of an operator made by ``adjoint()`` / ``transpose()``: take the CURRENT values of ``parent`` -- the operator it was
        made from, or one of the same pattern -- on the device (expv_mi_op_adjoint_refresh) and re-evaluate ``ishermitian`` /
        ``opnorm_inf``; bit-equal to ``parent.adjoint()`` made anew.  Another pattern with the same counts is the caller's error."""
        if not getattr(self, "_adj_how", 0):
            raise TypeError("refresh: only an operator made by adjoint() / transpose() refreshes from a parent")
        if not isinstance(parent, MIOperator):
            raise TypeError("refresh: the parent must be an MIOperator")
        _check(L.load().expv_mi_op_adjoint_refresh(self._h, parent._h), self.ctx._h)
        self._read_info()
        return self

    # ---- linear combinations of operators that exist (expv_mi_op_create_lincomb / expv_mi_op_lincomb_refresh) ----
    @staticmethod
    def _lincomb_args(terms, coefs, identity, who):
        terms, coefs = list(terms), list(coefs)
        for t in terms:
            if not isinstance(t, MIOperator):
                raise TypeError("%s: every term must be an MIOperator, not %s" % (who, type(t).__name__))
        if len(coefs) != len(terms):
            raise ValueError("%s: one coefficient per term expected (%d terms, %d coefficients)" % (who, len(terms), len(coefs)))
        for c in coefs + ([] if identity is None else [identity]):
            if not _is_scalar(c):
                raise TypeError("%s: a coefficient must be a scalar, not %s" % (who, type(c).__name__))
        pairs = np.zeros(2 * (len(coefs) + (identity is not None)), dtype=np.float64)
        for k, c in enumerate(coefs + ([] if identity is None else [identity])):
            c = complex(c)
            pairs[2 * k], pairs[2 * k + 1] = c.real, c.imag
        handles = (C.c_void_p * max(len(terms), 1))(*[t._h for t in terms])
        return terms, pairs, handles

    @staticmethod
    def lincomb(terms, coefs, identity=None):
        """``coefs[0] * terms[0] + ... + coefs[K-1] * terms[K-1] (+ identity * I)`` as a NEW, independent ``MIOperator`` on the
        terms' context (expv_mi_op_create_lincomb), K <= 8: the reference's ``expv(t, H0 + f*H1, b)`` and ``expv(t, A - sigma*I, b)``.
        Built on the device from what the terms store -- all sparse (of any birth, reordered or not) or all dense, one element type
        and size; the values never visit the host.  The pattern is the union of the terms' patterns (plus the diagonal when
        ``identity`` is given), whatever the values and coefficients are: cancelled entries stay stored.  The values are summed in
        term order, the identity last, nothing fused (include/expv_mi.h states the roundings).  This is the one-pass form for
        more than two terms: ``A + B + C`` builds ``A + B`` first.  ``recombine`` changes the coefficients, or follows the terms'
        values, at the cost of one kernel and a value refill.  As for ``adjoint()``: ``src`` is ``None``, ``astype`` is refused,
        ``update_values`` takes bare values in the result's own sorted-row order."""
        terms, pairs, handles = MIOperator._lincomb_args(terms, coefs, identity, "lincomb")
        if not terms:
            raise ValueError("lincomb: one term at least (the identity alone has no context, element type or size)")
        lib = L.load()
        h = C.c_void_p()
        ctx = terms[0].ctx
        _check(lib.expv_mi_op_create_lincomb(len(terms), handles, pairs.ctypes.data, L.LINCOMB_IDENTITY if identity is not None else 0,
                                             C.byref(h)), ctx._h)
        op = object.__new__(MIOperator)
        op.ctx, op.src, op._cb, op._matvec, op._h = ctx, None, None, None, h
        op._finalizer = weakref.finalize(op, lib.expv_mi_op_destroy, h)
        op._lc_terms, op._lc_identity = terms, identity
        op.src_dtype = terms[0].src_dtype
        if all(getattr(t, "_sp_format", None) is not None for t in terms):      # sparse: bare values refresh it in its own sorted-row order
            op._sp_format, op._sp_sorted = "csr", True
        op._read_info()
        return op

    def recombine(self, coefs, terms=None, identity=None):
        """Of an operator made by ``lincomb`` (or by ``+``, ``-``, ``*``, ``/``): new coefficients and the CURRENT values of the
        terms -- by default the ones kept from creation, else operators of the same patterns -- on the device
        (expv_mi_op_lincomb_refresh); ``ishermitian`` / ``opnorm_inf`` are re-evaluated.  Bit-equal to ``lincomb`` made anew.
        ``identity`` may only be given when the operator was created with one (its coefficient then defaults to the last one
        given).  Another pattern with the same counts is the caller's error."""
        kept = getattr(self, "_lc_terms", None)
        if kept is None:
            raise TypeError("recombine: only an operator made by lincomb() (or by + - * /) recombines")
        had = self._lc_identity is not None
        if identity is not None and not had:
            raise ValueError("recombine: the operator was made without the identity; its pattern holds no diagonal for one")
        if had and identity is None:
            identity = self._lc_identity
        terms, pairs, handles = MIOperator._lincomb_args(kept if terms is None else terms, coefs, identity, "recombine")
        _check(L.load().expv_mi_op_lincomb_refresh(self._h, len(terms), handles, pairs.ctypes.data), self.ctx._h)
        self._lc_terms, self._lc_identity = terms, identity
        self._read_info()
        return self

    __array_ufunc__ = None      # numpy leaves `array * A` and `scalar + A` to the methods below

    def _lc_other(self, other, sign, what):
        if not isinstance(other, MIOperator):
            hint = " (for a shift use MIOperator.lincomb([A], [1], identity=sigma))" if _is_scalar(other) else ""
            raise TypeError("%s: the other side must be an MIOperator, not %s%s" % (what, type(other).__name__, hint))
        return MIOperator.lincomb([self, other], [1.0, sign])

    def _lc_scaled(self, c, what):
        if not _is_scalar(c):
            raise TypeError("%s: the other side must be a scalar, not %s" % (what, type(c).__name__))
        return MIOperator.lincomb([self], [c])

    def __add__(self, other):
        """``A + B``: a new operator at every evaluation (the ``.H`` convention), ``lincomb([A, B], [1, 1])``"""
        return self._lc_other(other, 1.0, "A + B")

    def __radd__(self, other):
        return self._lc_other(other, 1.0, "B + A")

    def __sub__(self, other):
        """``A - B``: ``lincomb([A, B], [1, -1])``; ``A - A`` keeps the entries of ``A`` as stored zeros"""
        return self._lc_other(other, -1.0, "A - B")

    def __rsub__(self, other):
        raise TypeError("B - A: the other side must be an MIOperator, not %s" % type(other).__name__)

    def __neg__(self):
        """``-A``: ``lincomb([A], [-1])``"""
        return MIOperator.lincomb([self], [-1.0])

    def __mul__(self, c):
        """``A * c`` and ``c * A``: ``lincomb([A], [c])``"""
        return self._lc_scaled(c, "A * c")

    def __rmul__(self, c):
        return self._lc_scaled(c, "c * A")

    def __truediv__(self, c):
        """``A / c``: ``lincomb([A], [1 / c])`` -- the reciprocal is rounded first, then every entry multiplied"""
        if not _is_scalar(c):
            raise TypeError("A / c: the other side must be a scalar, not %s" % type(c).__name__)
        return MIOperator.lincomb([self], [1.0 / c])

    def __rtruediv__(self, c):
        raise TypeError("c / A: an operator has no reciprocal")

    def astype(self, dtype):
        dtype = _work_dtype(dtype)
        if dtype == self.dtype:
            return self
        if getattr(self, "_lc_terms", None) is not None:
            raise TypeError("an operator made by lincomb() (or by + - * /) keeps no source to convert: combine the converted terms, "
                            "MIOperator.lincomb([t.astype(dtype) for t in terms], coefs)")
        if getattr(self, "_adj_how", 0):
            raise TypeError("an operator made by adjoint() / transpose() keeps no source to convert: use parent.astype(dtype).adjoint() "
                            "(and refresh(parent.astype(dtype)) after the parent changes)")
        if getattr(self, "_sp_format", None) == "dia":      # rebuilt from the kept diagonals (on the device when they are there)
            key = "_as_" + dtype.name
            if not hasattr(self, key):
                data, offsets, n, align, _ = self._dia_parts
                setattr(self, key, MIOperator.from_dia(data, offsets, n, align, self.ctx, dtype=dtype))
            return getattr(self, key)
        if getattr(self, "_sp_format", None) == "bsr":      # rebuilt from the kept block arrays (on the device when they are there)
            key = "_as_" + dtype.name
            if not hasattr(self, key):
                ptr, idx, vals, n, base, compressed, order = self._bsr_parts
                setattr(self, key, MIOperator.from_bsr(ptr, idx, vals, n, base, compressed, order, self.ctx, dtype=dtype))
            return getattr(self, key)
        if getattr(self, "_sp_format", None) == "coo":      # rebuilt from the kept triplets (on the device when they are there)
            key = "_as_" + dtype.name
            if not hasattr(self, key):
                row, col, vals, n, base = self._coo_parts
                setattr(self, key, MIOperator.from_coo(row, col, vals, n, base, self.ctx, dtype=dtype))
            return getattr(self, key)
        if self.src is None or self._cb is not None:
            raise TypeError("cannot convert a matrix-free operator to another element type")
        key = "_as_" + dtype.name
        if not hasattr(self, key):
            setattr(self, key, MIOperator(self.src, self.ctx, dtype=dtype))
        return getattr(self, key)

    def matvec(self, x):
        """mul!(y, A, x)."""
        xa = _Arg(x, self.dtype)
        y = _empty_like(x, (self.shape[0],), self.dtype)
        ya = _Arg(y, self.dtype, writable=True)
        _check(L.load().expv_mi_op_apply(self._h, xa.ptr, xa.loc, ya.ptr, ya.loc), self.ctx._h)
        ya.finish()
        return y

    def matvec_complex(self, x, out=None):
        """mul!(y, A, x) for a REAL operator and complex vectors (expv_mi_op_apply_complex): the operator is read as it is stored, no
        promoted copy.  ``x``: numpy / torch (device) / DeviceArray, converted to the operator's complex type; ``out``: an optional
        vector of that type.  A complex operator raises (ArgumentError naming expv_mi_op_apply)."""
        Cd = _complex_of(self.dtype)
        xa = _Arg(x, Cd)
        y = _empty_like(x, (self.shape[0],), Cd) if out is None else out
        ya = _Arg(y, Cd, writable=True)
        if int(np.prod(xa.shape)) != self.shape[1] or int(np.prod(ya.shape)) != self.shape[0]:
            raise DimensionMismatch(f"mul!: A is {self.shape[0]} x {self.shape[1]}, x has {int(np.prod(xa.shape))}, y has {int(np.prod(ya.shape))}")
        _check(L.load().expv_mi_op_apply_complex(self._h, xa.ptr, xa.loc, ya.ptr, ya.loc), self.ctx._h)
        ya.finish()
        return y

    __matmul__ = matvec


def _torch_view(ptr, n, dt):
    import torch

    class _Shim:
        pass

    s = _Shim()
    s.__cuda_array_interface__ = {"shape": (n,), "typestr": np.dtype(dt).str,
                                  "data": (int(ptr), False), "version": 3}
    return torch.as_tensor(s, device="cuda")


def _wrapsum(a):
    """Content hash of an array's bytes (expv_mi_host_wrapsum): sum_i mix64(x_i ^ (i + 1) g) mod 2^64 over the 8-byte words, every
    word combined with its position and then put through a non-linear mixer -- any in-place permutation of the contents
    (A.data[:] = A.data[::-1], two swapped entries, also of mantissa-free values like the 1 / -2 of a stencil, at any distance)
    changes it.  An F-ordered matrix is read through its transpose (a C-contiguous view of the same memory: no copy)."""
    a = np.asarray(a)
    if a.ndim == 2 and a.flags.f_contiguous and not a.flags.c_contiguous:
        a = a.T
    a = np.ascontiguousarray(a)
    out = (C.c_uint64 * 2)()
    _check(L.load().expv_mi_host_wrapsum(a.ctypes.data if a.nbytes else None, a.nbytes, out))
    return (int(out[0]), int(out[1]))


def _fingerprint(A):
    """Cheap content fingerprint of a host matrix: shape, dtype, buffer addresses and a checksum of the values (and of the
    index arrays of a sparse matrix).  The reference reads A at call time (mul!(y, A, x)); an uploaded copy may only be
    reused while the caller's matrix is byte-for-byte what was uploaded."""
    if hasattr(A, "indptr") and hasattr(A, "indices"):
        return ("sp", A.format, A.shape, A.dtype.str, int(A.nnz), A.data.ctypes.data, A.indices.ctypes.data,
                A.indptr.ctypes.data, _wrapsum(A.data), _wrapsum(A.indices), _wrapsum(A.indptr))
    M = np.asarray(A)
    return ("dn", M.shape, M.dtype.str, M.ctypes.data, M.strides, _wrapsum(M))


def _as_operator(A, want_dtype=None, ctx=None):
    """Resolve the operator argument of an API call.  An explicit MIOperator is the way to reuse an upload across calls.
    Host matrices (scipy sparse / ndarray) passed directly are uploaded on first use and the upload is reused ONLY while
    (same object, same context, same content fingerprint) -- an in-place ``A.data[:] = ...`` / ``A *= dt`` between calls
    re-uploads, like the reference reading A at call time.  Device tensors are wrapped without a copy every time; that goes for
    sparse device tensors (``torch.sparse_csr`` / ``torch.sparse_csc``) too, whose operator is built anew at every call -- the
    device checks, the pattern's trip to the host planners, the fill of the stored forms; the plan cache spares a repeated
    pattern its ordering.  Reuse across calls is by an explicit ``MIOperator(A)`` (+ ``update_values``)."""
    if hasattr(A, "tocsr") and not hasattr(A, "indptr"):      # COO / DIA / LIL / ... : any scipy sparse matrix is an AbstractMatrix
        A = A.tocsr()
    if isinstance(A, MIOperator):
        op = A
    elif _is_torch_coo(A):          # coordinate triplets, coalesced or not, on either side (MIOperator.from_coo)
        op = MIOperator.from_coo(A, ctx=ctx)
    elif _is_torch_bsr(A):          # block-compressed, on either side (MIOperator.from_bsr)
        op = MIOperator.from_bsr(A, ctx=ctx)
    elif _is_torch(A):
        op = MIOperator(A, ctx)
    else:
        cache = getattr(_as_operator, "_cache", None)
        if cache is None:
            cache = _as_operator._cache = {}
        cobj = ctx or default_context()
        key = (id(A), id(cobj))
        fp = _fingerprint(A)
        ent = cache.get(key)
        same_obj = ent is not None and ent[0]() is A and ent[1].ctx is cobj
        if same_obj and ent[2] != fp and fp[0] == "sp" and ent[2][0] == "sp" and fp[1:8] == ent[2][1:8] and fp[9:] == ent[2][9:] \
                and A.format in ("csr", "csc") and A.has_sorted_indices and getattr(ent[1], "_sp_format", None) == A.format \
                and getattr(ent[1], "_sp_sorted", False) and ent[1].dtype == _work_dtype(A.dtype):
            # same arrays, same pattern (index checksums), other values: an in-place A.data[:] = ... between calls -- refill
            # the uploaded operator instead of building a new one
            op = ent[1].update_values(A)
            cache[key] = (ent[0], op, fp)
        elif ent is None or ent[0]() is not A or ent[2] != fp or ent[1].ctx is not cobj:
            op = MIOperator(A, cobj)
            try:
                cache[key] = (weakref.ref(A), op, fp)
            except TypeError:
                pass
            while len(cache) > 16:
                cache.pop(next(iter(cache)))
        else:
            op = ent[1]
    if want_dtype is not None:
        want = _work_dtype(want_dtype, op.dtype)      # conversions only go up (real -> complex, 32 -> 64 bit), never down
        if want != op.dtype:
            op = op.astype(want)
    return op


def _is_mixed(op, T):
    """a real operator whose complex counterpart is the vectors' work type T: what ``keep_real=True`` hands to the mixed entries"""
    return np.dtype(op.dtype).kind != "c" and np.dtype(T).kind == "c" and _complex_of(op.dtype) == np.dtype(T)


def _as_operator_for(A, T, ctx, keep_real):
    """_as_operator(A, T, ctx), except that with ``keep_real`` a real operator meeting complex vectors of its own precision is not
    promoted (no second, complex operator: a mixed call)"""
    if not keep_real:
        return _as_operator(A, T, ctx)
    op = _as_operator(A, None, ctx)
    return op if _is_mixed(op, T) else _as_operator(op, T, ctx)


def plan_cache(clear=False, capacity=None):
    """Ordering plans by pattern (expv_mi_plan_cache): creating a sparse operator whose pattern was seen before reuses the row
    ordering / patch plan worked out then.  Returns {"plans", "hits", "misses", "capacity"}; ``clear`` drops the stored plans,
    ``capacity`` sets how many patterns are kept (0 = off)."""
    out = (C.c_int64 * 4)()
    lib = L.load()
    if clear:
        _check(lib.expv_mi_plan_cache(1, 0, out))
    if capacity is not None:
        _check(lib.expv_mi_plan_cache(2, int(capacity), out))
    _check(lib.expv_mi_plan_cache(0, 0, out))
    return {"plans": int(out[0]), "hits": int(out[1]), "misses": int(out[2]), "capacity": int(out[3])}


def clear_operator_cache():
    """Drop every implicitly uploaded operator (see _as_operator)."""
    if hasattr(_as_operator, "_cache"):
        _as_operator._cache.clear()


# ---------------------------------------------------------------------------------------------
# KrylovSubspace                                                        arnoldi.jl:50-93
# ---------------------------------------------------------------------------------------------
class KrylovSubspace:
    """KrylovSubspace{T,U}(n, maxiter, augmented): V in HBM, H on the host (a live numpy view)."""

    def __init__(self, T, U=None, n=0, maxiter=30, augmented=0, ctx=None):
        lib = L.load()
        self.ctx = ctx or default_context()
        self.T = _work_dtype(T)
        self.U = _work_dtype(T if U is None else U)
        if self.U.kind == "c" and self.T.kind != "c":
            raise TypeError("U complex with T real")
        self.n = int(n)
        h = C.c_void_p()
        _check(lib.expv_mi_ks_create(self.ctx._h, _code(self.T), _code(self.U), self.n, int(maxiter),
                                     int(augmented), C.byref(h)), self.ctx._h)
        self._h = h
        self._finalizer = weakref.finalize(self, lib.expv_mi_ks_destroy, h)

    def _get(self):
        m, mi, aug, beta, wb = C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_int()
        _check(L.load().expv_mi_ks_get(self._h, C.byref(m), C.byref(mi), C.byref(aug), C.byref(beta), C.byref(wb)))
        return m.value, mi.value, aug.value, beta.value, bool(wb.value)

    m = property(lambda s: s._get()[0], lambda s, v: _check(L.load().expv_mi_ks_set_m(s._h, int(v)), s.ctx._h))
    maxiter = property(lambda s: s._get()[1])
    augmented = property(lambda s: s._get()[2])
    beta = property(lambda s: s._get()[3])
    wasbreakdown = property(lambda s: s._get()[4])

    @property
    def H(self):
        """Ks.H -- live view of the host matrix, (maxiter+1) x (maxiter + (augmented != 0))."""
        p, ld, nr, nc = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        _check(L.load().expv_mi_ks_H(self._h, C.byref(p), C.byref(ld), C.byref(nr), C.byref(nc)))
        buf = (C.c_char * (ld.value * nc.value * self.U.itemsize)).from_address(p.value)
        a = np.frombuffer(buf, dtype=self.U).reshape((nc.value, ld.value)).T
        return a[: nr.value, :]

    def getH(self):
        m, _, aug, _, _ = self._get()
        return self.H[: m + 1, : m + (aug != 0)]

    def V_host(self, col0=0, ncols=None):
        m, mi, aug, _, _ = self._get()
        if ncols is None:
            ncols = mi + 1 - col0
        out = np.empty((self.n + aug, ncols), dtype=self.T, order="F")
        _check(L.load().expv_mi_ks_V_download(self._h, int(col0), int(ncols), out.ctypes.data, max(out.shape[0], 1)),
               self.ctx._h)
        return out

    def getV(self):
        return self.V_host(0, self.m + 1)

    def resize(self, maxiter):
        _check(L.load().expv_mi_ks_resize(self._h, int(maxiter)), self.ctx._h)
        return self


def _opts(m=None, tol=1e-7, iop=0, init=0, ishermitian=None, ortho="auto", flags=0):
    o = L.ArnoldiOpts()
    L.load().expv_mi_arnoldi_opts_default(C.byref(o))
    o.flags = int(flags)
    o.m = int(m) if m is not None else 0
    o.tol = float(tol)
    o.iop = int(iop)
    o.init = int(init)
    o.ishermitian = -1 if ishermitian is None else int(bool(ishermitian))
    o.ortho = {"auto": L.ORTHO_AUTO, "mgs": L.ORTHO_MGS, "lowsync": L.ORTHO_LOWSYNC, "pipelined": L.ORTHO_PIPELINED}[ortho] \
        if isinstance(ortho, str) else int(ortho)
    return o


def arnoldi_(Ks, A, b, *, tol=1e-7, m=None, ishermitian=None, opnorm=None, iop=0, init=0, ortho="auto", defer_tail=True, keep_real=False):
    """arnoldi!(Ks, A, b; tol, m, ishermitian, opnorm, iop, init)  (arnoldi.jl:345-377).
    ``opnorm`` is accepted and ignored, like the reference.  ``keep_real=True``: a real operator under a complex subspace of its
    precision is used as it is stored (a mixed call, include/expv_mi.h) instead of being promoted through ``astype``."""
    op = _as_operator_for(A, Ks.T, Ks.ctx, keep_real)
    if op.dtype != Ks.T and not (keep_real and _is_mixed(op, Ks.T)):
        raise TypeError(f"operator eltype {op.dtype} does not fit KrylovSubspace{{{Ks.T}}}")
    ba = _Arg(b, Ks.T)
    if int(np.prod(ba.shape)) != op.shape[0]:
        raise DimensionMismatch(f"length(b) [{int(np.prod(ba.shape))}] == size(A,1) [{op.shape[0]}] doesn't hold")
    if ishermitian is None:
        ishermitian = op.ishermitian
    # (EXPV_MI_ARNOLDI_DEFER_TAIL: the closing pass is collected by whatever touches Ks next -- every accessor here is a library call)
    o = _opts(m, tol, iop, init, ishermitian, ortho, flags=1 if defer_tail else 0)
    _check(L.load().expv_mi_arnoldi(Ks._h, op._h, ba.ptr, ba.loc, C.byref(o)), Ks.ctx._h)
    return Ks


def lanczos_(Ks, A, b, *, tol=1e-7, m=None, opnorm=None, init=0, ortho="auto", keep_real=False):
    """lanczos!(Ks, A, b; tol, m)  (arnoldi.jl:456-490).  ``ortho="pipelined"``: the opt-in pipelined recurrence (include/expv_mi.h).
    ``keep_real``: as in arnoldi_."""
    op = _as_operator_for(A, Ks.T, Ks.ctx, keep_real)
    ba = _Arg(b, Ks.T)
    if int(np.prod(ba.shape)) != op.shape[0]:
        raise DimensionMismatch("length(b) == size(A,1) doesn't hold")
    o = _opts(m, tol, 0, init, True, ortho, flags=1)
    _check(L.load().expv_mi_lanczos(Ks._h, op._h, ba.ptr, ba.loc, C.byref(o)), Ks.ctx._h)
    return Ks


def arnoldi(A, b, *, m=None, ishermitian=None, **kw):
    """arnoldi(A, b; m = min(30, size(A,1)), ishermitian = LinearAlgebra.ishermitian(A), kwargs...)
    (arnoldi.jl:161-180).  ``keep_real``: as in arnoldi_."""
    bdt = _np_dtype_of(b)
    op = _as_operator(A, None)
    T = _work_dtype(op.dtype, bdt)
    op = _as_operator_for(op, T, None, kw.get("keep_real", False))
    if m is None:
        m = min(30, op.shape[0])
    if ishermitian is None:
        ishermitian = op.ishermitian
    U = _real_of(T) if ishermitian else T
    n = b.shape[0] if hasattr(b, "shape") else len(b)
    Ks = KrylovSubspace(T, U, n, m, 0, op.ctx)
    return arnoldi_(Ks, op, b, m=m, ishermitian=ishermitian, **kw)


# ---------------------------------------------------------------------------------------------
# expv / phiv                                                     krylov_phiv.jl:125-653
# ---------------------------------------------------------------------------------------------
def _t_parts(t):
    tc = isinstance(t, (complex, np.complexfloating))
    return float(np.real(t)), float(np.imag(t)) if tc else 0.0, tc


def expv_(w, t, Ks):
    """expv!(w, t, Ks)  (krylov_phiv.jl:200-280)."""
    tr, ti, tc = _t_parts(t)
    wdt = _np_dtype_of(w)
    if (tc or Ks.T.kind == "c") and wdt.kind != "c":
        raise TypeError("InexactError: w must be complex when t or the basis is complex")
    wa = _Arg(w, _complex_of(Ks.T) if wdt.kind == "c" else _real_of(Ks.T), writable=True)   # (the basis' precision; a numpy w of another one is filled through a copy)
    if wa.shape[0] != Ks.n + Ks.augmented:
        raise AssertionError("Dimension mismatch")
    _check(L.load().expv_mi_expv_ks(Ks._h, tr, ti, wa.ptr, wa.loc, _code(wa.dtype)), Ks.ctx._h)
    wa.finish()
    return w


def expv(t, A, b=None, *, mode="happy_breakdown", **kw):
    """expv(t, A, b; mode = :happy_breakdown | :error_estimate, kwargs...)  (krylov_phiv.jl:125-160)."""
    if isinstance(A, KrylovSubspace):       # expv(t, Ks)  (:161-168)
        Ks = A
        w = np.empty(Ks.n, dtype=_complex_of(Ks.T) if _t_parts(t)[2] else Ks.T, order="F")
        return expv_(w, t, Ks)
    tr, ti, tc = _t_parts(t)
    tdt = np.complex64 if tc else np.float32        # (weak: t never widens the work type; the RESULT type follows _t_dtype(t))
    op = _as_operator(A, None)
    bdt = _np_dtype_of(b)
    n = b.shape[0]
    if mode == "happy_breakdown":
        # expv(t, A, b) = arnoldi + expv! (krylov_phiv.jl:135-144) as ONE library call: the subspace is
        # private to the call, so the library reuses its workspace and skips v_{m+1} / H[m+1, m]
        T = _work_dtype(op.dtype, bdt)
        # keep_real=True: a real operator meeting a complex b stays as it is stored (expv_mi_expv_realop: no promoted copy)
        opT = _as_operator_for(op, T, None, kw.get("keep_real", False))
        mixed = opT.dtype != T
        extra = set(kw) - {"m", "tol", "iop", "ishermitian", "ortho", "opnorm", "out", "keep_real"}
        if extra:
            raise TypeError(f"unexpected keyword(s) {sorted(extra)}")
        ish = kw.get("ishermitian")
        o = _opts(kw.get("m", min(30, op.shape[0])), kw.get("tol", 1e-7), kw.get("iop", 0), 0,
                  opT.ishermitian if ish is None else ish, kw.get("ortho", "auto"))
        w = kw.get("out")           # optional preallocated result (not in the reference: saves the allocation)
        if w is None:
            w = _empty_like(b, (n,), _work_dtype(tdt, T))
        ba, wa = _Arg(b, T), _Arg(w, _work_dtype(tdt, T), writable=True)
        if int(np.prod(ba.shape)) != op.shape[0]:
            raise DimensionMismatch(f"length(b) [{int(np.prod(ba.shape))}] == size(A,1) [{op.shape[0]}] doesn't hold")
        st = L.ExpvStats()
        if mixed:
            _check(L.load().expv_mi_expv_realop(opT.ctx._h, opT._h, tr, ti, ba.ptr, ba.loc, wa.ptr, wa.loc,
                                                C.byref(o), C.byref(st)), opT.ctx._h)
        else:
            _check(L.load().expv_mi_expv(opT.ctx._h, opT._h, tr, ti, ba.ptr, ba.loc, wa.ptr, wa.loc, _code(wa.dtype),
                                         C.byref(o), C.byref(st)), opT.ctx._h)
        wa.finish()
        if kw.get("out") is None:
            w = _round_to(w, _ref_dtype(_t_dtype(t), getattr(op, "src_dtype", op.dtype), bdt))
        expv.last_stats = {"m": st.m_used, "wasbreakdown": bool(st.wasbreakdown), "matvecs": st.matvecs, "beta": st.beta,
                           "path": [k for k, v in L.PATH_FLAGS.items() if st.path_flags & v],
                           "fa2_pipelined": bool(st.path_flags & L.PATH_FA2_PIPELINED),
                           "real_operator": bool(st.path_flags & L.PATH_REAL_OPERATOR)}
        return w
    if mode == "error_estimate":        # _expv_ee  (:145-160)
        m = kw.pop("m", min(30, op.shape[0]))
        tol = kw.pop("tol", 1e-7)
        rtol = kw.pop("rtol", math.sqrt(tol))
        ish = kw.pop("ishermitian", None)
        if ish is None:
            ish = op.ishermitian
        T = _work_dtype(tdt, op.dtype, bdt)
        opT = _as_operator(op, T)
        if not ish:
            raise RuntimeError("Error estimation not yet available for non-Hermitian matrices.")
        Ks = KrylovSubspace(T, _real_of(T), op.shape[0], m, 0, op.ctx)
        w = _empty_like(b, (n,), T)
        ba, wa = _Arg(b, T), _Arg(w, T, writable=True)
        _check(L.load().expv_mi_expv_error_estimate(Ks._h, opT._h, tr, ti, ba.ptr, ba.loc, wa.ptr, wa.loc,
                                                    float(tol), float(rtol), int(m), int(bool(ish))), Ks.ctx._h)
        wa.finish()
        expv.last_subspace = Ks
        return _round_to(w, _ref_dtype(_t_dtype(t), getattr(op, "src_dtype", op.dtype), bdt))     # same result type in every mode
    raise ValueError(f"Unknown Krylov iteration termination mode, {mode}")     # ArgumentError (:132)


def _host_view(x):
    """a torch tensor in host memory as the numpy array that shares its storage (anything else as it is)"""
    return x.detach().numpy() if _is_torch(x) and not x.is_cuda else x


_TAYLOR_INFO = ("m", "s", "applications", "early_stages", "launches", "host_reads", "path", "nonfinite_stage")


def expv_taylor_(w, t, A, b, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """w <- exp(t A) b by the truncated Taylor series of Al-Mohy & Higham (expv_mi_expv_taylor; the reference's second expv
    algorithm, ext/ExponentialUtilitiesStaticArraysExt.jl:124-163): no Krylov basis, no inner product, three work vectors, the
    stopping rule decided on the device.  ``A``: anything an API call takes as an operator; ``b`` / ``w``: numpy, torch (either
    side for ``b``), DeviceArray; they may be the same array.  ``precision``: None / 0 = the working precision of the operator's
    real type, 1 = the 2^-24 table also for 64-bit operators.  ``max_matvecs`` > 0 refuses a call that would need more operator
    applications (ArgumentError naming alpha, m*, s).  ``opnorm``: a bound on opnorm(A, Inf), needed by matrix-free operators
    only.  A complex ``t`` needs a complex operator.  ``return_info``: also return the dictionary kept in
    ``expv_taylor.last_info`` (m, s, applications, early_stages, launches, host_reads, path: 1 fused / 2 mul! + update,
    nonfinite_stage, alpha, mu, normF)."""
    tr, ti, _ = _t_parts(t)
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(b))
    opT = _as_operator(op, T)
    ba, wa = _Arg(_host_view(b), T), _Arg(_host_view(w), T, writable=True)
    n = opT.shape[0]
    if int(np.prod(ba.shape)) != n:
        raise DimensionMismatch(f"length(b) [{int(np.prod(ba.shape))}] == size(A,1) [{n}] doesn't hold")
    if int(np.prod(wa.shape)) != n:
        raise DimensionMismatch(f"length(w) [{int(np.prod(wa.shape))}] == size(A,1) [{n}] doesn't hold")
    info, dinfo = (C.c_int64 * 8)(), (C.c_double * 4)()
    _check(L.load().expv_mi_expv_taylor(opT.ctx._h, opT._h, tr, ti, ba.ptr, ba.loc, wa.ptr, wa.loc, int(precision or 0),
                                        int(max_matvecs), 0.0 if opnorm is None else float(opnorm), info, dinfo), opT.ctx._h)
    wa.finish()
    d = dict(zip(_TAYLOR_INFO, (int(v) for v in info)))
    d.update(alpha=float(dinfo[0]), mu=complex(dinfo[1], dinfo[2]) if T.kind == "c" else float(dinfo[1]), normF=float(dinfo[3]))
    expv_taylor.last_info = d
    return (w, d) if return_info else w


def expv_taylor(t, A, b, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """exp(t A) b by the truncated Taylor series (see expv_taylor_): the result lives where ``b`` does and has the element type
    the device worked in (the operator's, complex when ``b`` is)."""
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(b))
    if _is_torch(b) and not b.is_cuda:
        import torch
        w = torch.empty(b.shape[0], dtype=_torch_dtype(T))
    else:
        w = _empty_like(b, (b.shape[0],), T)
    return expv_taylor_(w, t, op, b, precision=precision, max_matvecs=max_matvecs, opnorm=opnorm, return_info=return_info, ctx=ctx)


def expv_taylor_realop_(w, t, A, b, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """w <- exp(t A) b for a REAL operator, a complex (or real) ``t`` and complex vectors (expv_mi_expv_taylor_realop): the
    Schroedinger / wave propagation exp(-i t H) b with a real sparse H.  The operator is used as it is stored -- no promoted complex
    copy -- and the series, its plan and its roundings are those of expv_taylor_ (on an operator with a fused form the values are
    those of expv_taylor on the promoted operator, element for element).  ``A``: anything real an API call takes as an operator
    (a complex one is refused: ArgumentError naming expv_mi_expv_taylor).  ``b``: real or complex, numpy / torch (either side) /
    DeviceArray, converted to the operator's precision; a real ``b`` is widened on the device.  ``w``: complex, of the operator's
    precision; it may be ``b`` itself when ``b`` is complex.  The other arguments and the dictionary kept in
    ``expv_taylor_realop.last_info`` are those of expv_taylor_ (path 2 applies the operator twice per term: to the real and to the
    imaginary plane)."""
    tr, ti, _ = _t_parts(t)
    op = _as_operator(A, None, ctx)
    Cd = _complex_of(op.dtype)
    bdt = _np_dtype_of(b)
    ba = _Arg(_host_view(b), Cd if (bdt.kind == "c" or np.dtype(op.dtype).kind == "c") else _real_of(op.dtype))
    wa = _Arg(_host_view(w), Cd, writable=True)
    n = op.shape[0]
    if int(np.prod(ba.shape)) != n:
        raise DimensionMismatch(f"length(b) [{int(np.prod(ba.shape))}] == size(A,1) [{n}] doesn't hold")
    if int(np.prod(wa.shape)) != n:
        raise DimensionMismatch(f"length(w) [{int(np.prod(wa.shape))}] == size(A,1) [{n}] doesn't hold")
    info, dinfo = (C.c_int64 * 8)(), (C.c_double * 4)()
    _check(L.load().expv_mi_expv_taylor_realop(op.ctx._h, op._h, tr, ti, ba.ptr, ba.loc, _code(ba.dtype), wa.ptr, wa.loc, int(precision or 0),
                                               int(max_matvecs), 0.0 if opnorm is None else float(opnorm), info, dinfo), op.ctx._h)
    wa.finish()
    d = dict(zip(_TAYLOR_INFO, (int(v) for v in info)))
    d.update(alpha=float(dinfo[0]), mu=float(dinfo[1]), normF=float(dinfo[3]))
    expv_taylor_realop.last_info = d
    return (w, d) if return_info else w


def expv_taylor_realop(t, A, b, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """exp(t A) b for a real operator with a complex time and / or a complex vector (see expv_taylor_realop_): the result is complex,
    of the operator's precision, and lives where ``b`` does."""
    op = _as_operator(A, None, ctx)
    Cd = _complex_of(op.dtype)
    if _is_torch(b) and not b.is_cuda:
        import torch
        w = torch.empty(b.shape[0], dtype=_torch_dtype(Cd))
    else:
        w = _empty_like(b, (b.shape[0],), Cd)
    return expv_taylor_realop_(w, t, op, b, precision=precision, max_matvecs=max_matvecs, opnorm=opnorm, return_info=return_info, ctx=ctx)


_TAYLOR_BLOCK_INFO = ("m", "s", "applications_total", "worked_launches", "launches", "host_reads", "path", "nonfinite_columns")


def _block_layout(n, p, s0, s1):
    """(layout, ld) of an n x p block whose element (i, k) lies s0 * i + s1 * k elements from the first, or None when neither
    dimension has a unit stride (or the other one's stride is shorter than a row / column)"""
    if n == 0 or p == 0:      # nothing to address
        return L.BLOCK_ROW_MAJOR, max(p, 1)
    if s1 == 1 and (n <= 1 or s0 >= p):
        return L.BLOCK_ROW_MAJOR, max(s0 if n > 1 else p, p, 1)
    if s0 == 1 and (p <= 1 or s1 >= n):
        return L.BLOCK_COL_MAJOR, max(s1 if p > 1 else n, n, 1)
    if p <= 1 and s0 >= 1:      # one column at a row stride
        return L.BLOCK_ROW_MAJOR, s0
    if n <= 1 and s1 >= 1:
        return L.BLOCK_COL_MAJOR, s1
    return None


class _BlockArg:
    """A caller's 2-D block for expv_mi_expv_taylor_block: (pointer, loc, leading dimension, layout) of the array AS IT LIES in
    memory -- a C-ordered numpy array or a contiguous torch (n, p) tensor goes in as ROW_MAJOR, nothing is transposed.  An input of
    another element type, or one without a unit stride, is copied; an output like that is computed into a copy and written back
    (numpy) or refused (torch)."""

    def __init__(self, x, dtype, writable=False):
        self.dtype = np.dtype(dtype)
        self.back = None
        if isinstance(x, DeviceArray):
            if x.dtype != self.dtype:
                raise TypeError(f"device array has dtype {x.dtype}, need {self.dtype}")
            if x.ndim != 2:
                raise DimensionMismatch("expv_taylor_block takes a 2-D block (expv_taylor takes a vector)")
            self.ptr, self.loc, self.shape, self.keep = x.ptr, L.DEVICE, x.shape, x
            self.layout, self.ld = L.BLOCK_COL_MAJOR, max(x.shape[0], 1)
            return
        if _is_torch(x) and x.is_cuda:
            import torch
            if x.dim() != 2:
                raise DimensionMismatch("expv_taylor_block takes a 2-D block (expv_taylor takes a vector)")
            want = _torch_dtype(self.dtype)
            if x.dtype != want:
                if writable:
                    raise TypeError(f"output tensor must be {want}")
                x = x.to(want)
            n, p = x.shape
            lay = _block_layout(n, p, x.stride(0), x.stride(1))
            if lay is None:
                if writable:
                    raise TypeError("output block needs a unit stride along one dimension")
                x = x.contiguous()
                lay = _block_layout(n, p, x.stride(0), x.stride(1))
            self.layout, self.ld = lay
            st = torch.cuda.current_stream(x.device)      # (see _Arg: the library works on its own stream)
            if not st.query():
                st.synchronize()
            self.ptr, self.loc, self.shape, self.keep = x.data_ptr(), L.DEVICE, (int(n), int(p)), x
            return
        a = np.asarray(_host_view(x))
        if a.ndim != 2:
            raise DimensionMismatch("expv_taylor_block takes a 2-D block (expv_taylor takes a vector)")
        n, p = a.shape
        isz = self.dtype.itemsize

        def lay_of(a):
            if a.dtype != self.dtype or a.strides[0] % isz or a.strides[1] % isz:
                return None
            return _block_layout(n, p, a.strides[0] // isz, a.strides[1] // isz)
        lay = lay_of(a)
        if lay is None:
            order = "C" if a.flags.c_contiguous else "F"
            if writable:
                self.back = a
                a = np.empty(a.shape, dtype=self.dtype, order=order)
            else:
                a = np.array(a, dtype=self.dtype, order=order)
            lay = lay_of(a)
        self.layout, self.ld = lay
        self.ptr, self.loc, self.shape, self.keep, self.host = a.ctypes.data, L.HOST, (int(n), int(p)), a, a

    def finish(self):
        if self.back is not None:
            if np.iscomplexobj(self.host) and not np.iscomplexobj(self.back):
                raise TypeError("InexactError: complex result into a real array")
            self.back[...] = self.host


def expv_taylor_block_(W, t, A, B, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """W <- exp(t A) B for an n x p block B by the truncated Taylor series (expv_mi_expv_taylor_block): p independent problems of
    expv_taylor_ that share every pass over the operator.  Column k of W is bit for bit ``expv_taylor(t, A, B[:, k])``.  ``B`` /
    ``W``: 2-D numpy arrays (either order, or a view with one unit stride), torch tensors (either side; a contiguous (n, p) tensor
    goes in row-major as it is) or DeviceArray; W may be B.  ``precision``, ``max_matvecs`` (compared with m* s, the cost of one
    column), ``opnorm`` and ``t`` as in expv_taylor_.  Operators with a fused term kernel run in panels of 8 columns; a column that
    has stopped is masked but keeps being streamed until the last column of its panel stops.  ``return_info``: also return the
    dictionary kept in ``expv_taylor_block.last_info``: m, s, applications_total, worked_launches, launches, host_reads, path
    (1 block kernel / 2 column by column), nonfinite_columns, alpha, mu, normF_max and the per-column lists applications,
    early_stages, nonfinite_stage, normF."""
    tr, ti, _ = _t_parts(t)
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(B))
    opT = _as_operator(op, T)
    ba, wa = _BlockArg(B, T), _BlockArg(W, T, writable=True)      # (W is B resolves to the same pointer, ld and layout)
    n = opT.shape[0]
    if ba.shape[0] != n:
        raise DimensionMismatch(f"size(B,1) [{ba.shape[0]}] == size(A,1) [{n}] doesn't hold")
    if wa.shape != ba.shape:
        raise DimensionMismatch(f"size(W) [{wa.shape}] == size(B) [{ba.shape}] doesn't hold")
    p = ba.shape[1]
    info, dinfo = (C.c_int64 * 8)(), (C.c_double * 4)()
    cinfo, cnorm = (C.c_int64 * max(3 * p, 1))(), (C.c_double * max(p, 1))()
    _check(L.load().expv_mi_expv_taylor_block(opT.ctx._h, opT._h, tr, ti, ba.ptr, ba.ld, p, ba.layout, ba.loc, wa.ptr, wa.ld, wa.layout,
                                              wa.loc, int(precision or 0), int(max_matvecs), 0.0 if opnorm is None else float(opnorm),
                                              info, dinfo, cinfo, cnorm), opT.ctx._h)
    wa.finish()
    d = dict(zip(_TAYLOR_BLOCK_INFO, (int(v) for v in info)))
    d.update(alpha=float(dinfo[0]), mu=complex(dinfo[1], dinfo[2]) if T.kind == "c" else float(dinfo[1]), normF_max=float(dinfo[3]),
             applications=[int(cinfo[3 * k]) for k in range(p)], early_stages=[int(cinfo[3 * k + 1]) for k in range(p)],
             nonfinite_stage=[int(cinfo[3 * k + 2]) for k in range(p)], normF=[float(cnorm[k]) for k in range(p)])
    expv_taylor_block.last_info = d
    return (W, d) if return_info else W


def expv_taylor_block(t, A, B, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """exp(t A) B for an n x p block (see expv_taylor_block_): the result lives where ``B`` does, in B's memory order, and has the
    element type the device worked in."""
    if len(B.shape) != 2:
        raise DimensionMismatch("expv_taylor_block takes a 2-D block (expv_taylor takes a vector)")
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(B))
    shape = (int(B.shape[0]), int(B.shape[1]))
    if isinstance(B, DeviceArray):
        W = DeviceArray(shape, T, B.ctx)
    elif _is_torch(B):
        import torch
        rowmajor = B.stride(1) == 1 or B.stride(0) != 1
        W = (torch.empty(shape, dtype=_torch_dtype(T), device=B.device) if rowmajor
             else torch.empty((shape[1], shape[0]), dtype=_torch_dtype(T), device=B.device).t())
    else:
        Bn = np.asarray(B)
        W = np.empty(shape, dtype=T, order="F" if (Bn.flags.f_contiguous and not Bn.flags.c_contiguous) or
                     (not Bn.flags.c_contiguous and Bn.strides[0] == Bn.itemsize) else "C")
    return expv_taylor_block_(W, t, op, B, precision=precision, max_matvecs=max_matvecs, opnorm=opnorm, return_info=return_info, ctx=ctx)


_TAYLOR_GRID_INFO = _TAYLOR_INFO + ("accumulate_launches", "qmax")


def _grid_multipliers(ts, t):
    """(r, t'): the multipliers r_k = |ts_k| as a float64 array of its own and ``t`` with the common sign of ``ts`` folded in"""
    r = np.array(_host_view(ts.detach().cpu() if _is_torch(ts) else ts), dtype=np.float64).ravel()
    if np.any(r > 0) and np.any(r < 0):
        raise L.ExpvMIError(2, "expv_taylor_grid: ts must be all >= 0 or all <= 0 (the sign is folded into t)")
    if np.any(r < 0):
        r, t = -r, -t
    return np.ascontiguousarray(r), t


def expv_taylor_grid_(W, ts, A, b, *, t=1.0, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """W[:, k] <- exp(ts[k] t A) b for a vector of real times in ONE sweep of the truncated Taylor series of expv_taylor_
    (expv_mi_expv_taylor_grid): with R = max |ts|, the call is expv_taylor_'s for R t -- its mu, alpha, m*, s, its F and v,
    operation for operation -- and every other output is read off the terms of the stage it falls into, at no extra pass over
    the operator.  Columns with |ts[k]| = R are bit for bit ``expv_taylor(R t, A, b)``; ts[k] = 0 gives b.  ``ts``: real, all
    >= 0 or all <= 0 (the sign goes into ``t``; mixed signs are an ArgumentError), any order, duplicates allowed, not modified.
    ``W``: an (n, len(ts)) block as expv_taylor_block_ takes it; it may not overlap ``b``.  ``precision``, ``max_matvecs``
    (against m* s), ``opnorm`` and a complex ``t`` as in expv_taylor_.  ``return_info``: also return the dictionary kept in
    ``expv_taylor_grid.last_info``: the keys of expv_taylor_ (applications = term launches that did work, shared by all outputs),
    accumulate_launches, qmax (the most interior outputs of one stage) and the per-output lists stage (-1 for ts[k] = 0), terms,
    kind (0 = b, 1 = interior, 2 = stage end)."""
    r, t = _grid_multipliers(ts, t)
    tr, ti, _ = _t_parts(t)
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(b))
    opT = _as_operator(op, T)
    ba, wa = _Arg(_host_view(b), T), _BlockArg(W, T, writable=True)
    n, q = opT.shape[0], int(r.size)
    if int(np.prod(ba.shape)) != n:
        raise DimensionMismatch(f"length(b) [{int(np.prod(ba.shape))}] == size(A,1) [{n}] doesn't hold")
    if wa.shape != (n, q):
        raise DimensionMismatch(f"size(W) [{wa.shape}] == (size(A,1), length(ts)) [{(n, q)}] doesn't hold")
    info, dinfo = (C.c_int64 * 10)(), (C.c_double * 4)()
    cinfo = (C.c_int64 * max(3 * q, 1))()
    _check(L.load().expv_mi_expv_taylor_grid(opT.ctx._h, opT._h, tr, ti, r.ctypes.data_as(C.POINTER(C.c_double)), q, ba.ptr, ba.loc, wa.ptr,
                                             wa.ld, wa.layout, wa.loc, int(precision or 0), int(max_matvecs),
                                             0.0 if opnorm is None else float(opnorm), info, dinfo, cinfo), opT.ctx._h)
    wa.finish()
    d = dict(zip(_TAYLOR_GRID_INFO, (int(v) for v in info)))
    d.update(alpha=float(dinfo[0]), mu=complex(dinfo[1], dinfo[2]) if T.kind == "c" else float(dinfo[1]), normF=float(dinfo[3]),
             stage=[int(cinfo[3 * k]) for k in range(q)], terms=[int(cinfo[3 * k + 1]) for k in range(q)],
             kind=[int(cinfo[3 * k + 2]) for k in range(q)])
    expv_taylor_grid.last_info = d
    return (W, d) if return_info else W


def expv_taylor_grid(ts, A, b, *, t=1.0, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """exp(ts[k] t A) b for a vector of real times (see expv_taylor_grid_): an (n, len(ts)) result that lives where ``b`` does --
    Fortran order for numpy, a contiguous (n, q) tensor for torch -- in the element type the device worked in.  A scalar ``ts``
    returns the vector ``expv_taylor(ts * t, A, b)``, bit for bit."""
    if np.ndim(_host_view(ts) if not (_is_torch(ts) and ts.is_cuda) else ts.cpu()) == 0:
        return expv_taylor(float(ts) * t, A, b, precision=precision, max_matvecs=max_matvecs, opnorm=opnorm, return_info=return_info, ctx=ctx)
    _grid_multipliers(ts, t)      # (mixed signs: refused before anything is created)
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(b))
    shape = (int(b.shape[0]), int(np.size(_host_view(ts) if not _is_torch(ts) else ts.cpu())))
    if isinstance(b, DeviceArray):
        W = DeviceArray(shape, T, b.ctx)
    elif _is_torch(b):
        import torch
        W = torch.empty(shape, dtype=_torch_dtype(T), device=b.device)
    else:
        W = np.empty(shape, dtype=T, order="F")
    return expv_taylor_grid_(W, ts, op, b, t=t, precision=precision, max_matvecs=max_matvecs, opnorm=opnorm, return_info=return_info, ctx=ctx)


def host_taylor_grid_plan(s, r):
    """The classification of expv_taylor_grid's outputs for ``s`` stages and multipliers ``r`` >= 0 (expv_mi_host_taylor_grid_plan;
    host only): (stage, rho, kind) as int64 / float64 / int32 arrays -- x = s (r / max r), stage = max(ceil(x) - 1, 0), rho = x - stage;
    kind 0: r = 0 (stage -1, rho 0), 2: rho = 1 (a stage end), 1: interior."""
    r = np.ascontiguousarray(np.asarray(r, dtype=np.float64).ravel())
    q = int(r.size)
    stage, rho, kind = np.zeros(max(q, 1), dtype=np.int64), np.zeros(max(q, 1), dtype=np.float64), np.zeros(max(q, 1), dtype=np.int32)
    _check(L.load().expv_mi_host_taylor_grid_plan(int(s), r.ctypes.data_as(C.POINTER(C.c_double)), q, stage.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  rho.ctypes.data_as(C.POINTER(C.c_double)), kind.ctypes.data_as(C.POINTER(C.c_int))))
    return stage[:q], rho[:q], kind[:q]


def phiv_taylor_(w, t, A, B, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """w <- phi_0(tA) u_0 + t phi_1(tA) u_1 + ... + t^p phi_p(tA) u_p for B = [u_0 ... u_p] (the result of phiv_timestep(t, A, B)) by the
    truncated Taylor series on Al-Mohy & Higham's augmented matrix (expv_mi_phiv_taylor): no Krylov basis, no host exponential, three
    work vectors of n elements.  ``B``: an n x (p + 1) block, p <= 8, numpy (either order), torch (either side) or DeviceArray, taken
    as it lies in memory; ``w``: a vector as in expv_taylor_, which may be column 0 of B.  ``precision``, ``max_matvecs``, ``opnorm``
    and ``t`` as in expv_taylor_.  One column is expv_taylor_ bit for bit.  ``return_info``: also return the dictionary kept in
    ``phiv_taylor.last_info``: the keys of expv_taylor_ plus ``nu`` (the scaling of the forcing columns behind alpha) and ``U``
    (max |u_k[i]|, k >= 1)."""
    tr, ti, _ = _t_parts(t)
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(B))
    opT = _as_operator(op, T)
    ba, wa = _BlockArg(B, T), _Arg(_host_view(w), T, writable=True)
    n = opT.shape[0]
    if ba.shape[0] != n:
        raise DimensionMismatch(f"size(B,1) [{ba.shape[0]}] == size(A,1) [{n}] doesn't hold")
    if int(np.prod(wa.shape)) != n:
        raise DimensionMismatch(f"length(w) [{int(np.prod(wa.shape))}] == size(A,1) [{n}] doesn't hold")
    info, dinfo = (C.c_int64 * 8)(), (C.c_double * 8)()
    _check(L.load().expv_mi_phiv_taylor(opT.ctx._h, opT._h, tr, ti, ba.ptr, ba.ld, ba.shape[1], ba.layout, ba.loc, wa.ptr, wa.loc,
                                        int(precision or 0), int(max_matvecs), 0.0 if opnorm is None else float(opnorm), info, dinfo),
           opT.ctx._h)
    wa.finish()
    d = dict(zip(_TAYLOR_INFO, (int(v) for v in info)))
    d.update(alpha=float(dinfo[0]), mu=complex(dinfo[1], dinfo[2]) if T.kind == "c" else float(dinfo[1]), normF=float(dinfo[3]),
             nu=float(dinfo[4]), U=float(dinfo[5]))
    phiv_taylor.last_info = d
    return (w, d) if return_info else w


def phiv_taylor(t, A, B, *, precision=None, max_matvecs=0, opnorm=None, return_info=False, ctx=None):
    """sum_k t^k phi_k(tA) B[:, k] by the truncated Taylor series (see phiv_taylor_): a vector that lives where ``B`` does and has the
    element type the device worked in."""
    if len(B.shape) != 2:
        raise DimensionMismatch("phiv_taylor takes a 2-D block B = [u_0 ... u_p]")
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(B))
    n = int(B.shape[0])
    if isinstance(B, DeviceArray):
        w = DeviceArray((n,), T, B.ctx)
    elif _is_torch(B):
        import torch
        w = torch.empty(n, dtype=_torch_dtype(T), device=B.device)
    else:
        w = np.empty(n, dtype=T)
    return phiv_taylor_(w, t, op, B, precision=precision, max_matvecs=max_matvecs, opnorm=opnorm, return_info=return_info, ctx=ctx)


def host_taylor_theta(m, precision=0):
    """theta_m (m = 1 .. 55) of the truncated-Taylor tables (expv_mi_host_taylor_theta; host only): precision 0 = tol 2^-53,
    1 = tol 2^-24."""
    th = C.c_double(0.0)
    _check(L.load().expv_mi_host_taylor_theta(int(precision), int(m), C.byref(th)))
    return float(th.value)


def host_taylor_params(alpha, precision=0):
    """(m*, s) of expv_taylor for alpha = |t| opnorm(A - mu I, Inf) (expv_mi_host_taylor_params; host only)."""
    m, s = C.c_int(0), C.c_int64(0)
    _check(L.load().expv_mi_host_taylor_params(int(precision), float(alpha), C.byref(m), C.byref(s)))
    return int(m.value), int(s.value)


def host_taylor_params_power(alpha1, d, precision=0):
    """(m*, s, p_used) of the reference's whole parameter search (expv_mi_host_taylor_params_power; host only): ``alpha1`` =
    |t| opnorm(A - mu I, Inf), ``d`` = the eight values d_2 .. d_9, d_p = |t| ||(A - mu I)^p||^(1/p).  p_used = 0: the first branch."""
    dd = np.ascontiguousarray(d, dtype=np.float64)
    if dd.shape != (8,):
        raise DimensionMismatch("host_taylor_params_power: d holds the eight values d_2 .. d_9")
    m, s, pu = C.c_int(0), C.c_int64(0), C.c_int(0)
    _check(L.load().expv_mi_host_taylor_params_power(int(precision), float(alpha1), dd.ctypes.data_as(C.POINTER(C.c_double)), C.byref(m),
                                                     C.byref(s), C.byref(pu)))
    return int(m.value), int(s.value), int(pu.value)


def host_normest_signs(n, col, attempt):
    """The +-1 signs (int8) the norm estimator draws for natural rows 0 .. n - 1 of column ``col`` at draw ``attempt``
    (expv_mi_host_normest_signs; host only): what a restatement of ``MIOperator.norm_power`` is pinned to."""
    out = np.empty(max(int(n), 0), dtype=np.int8)
    _check(L.load().expv_mi_host_normest_signs(int(n), int(col), int(attempt), out.ctypes.data if out.size else None))
    return out


_TAYLOR_POWER_INFO = _TAYLOR_INFO + ("p_used", "normest_applications", "normest_reads", "temporary_adjoint")


def expv_taylor_power_(w, t, A, b, *, adjoint=None, precision=None, max_matvecs=0, return_info=False, ctx=None):
    """w <- exp(t A) b by the truncated Taylor series with the reference's WHOLE parameter search (expv_mi_expv_taylor_power): when
    alpha = |t| opnorm(A - mu I, Inf) is above the cheap threshold, d_p = |t| ||(A - mu I)^p||^(1/p), p = 2 .. 9, are estimated on the
    device (``MIOperator.norm_power``) and (m*, s) come from ``host_taylor_params_power`` -- orders of magnitude fewer operator
    applications for a non-normal ``A``.  Below the threshold the call is ``expv_taylor_``, bit for bit.  ``adjoint``: an operator of
    ``A'`` (``A.adjoint()``), or None: a Hermitian ``A`` serves as its own, otherwise one is made for the call.  Stored operators
    only.  Everything else as ``expv_taylor_``; the info dictionary (``expv_taylor_power.last_info``) adds p_used,
    normest_applications, normest_reads, temporary_adjoint and d (d_2 .. d_9)."""
    tr, ti, _ = _t_parts(t)
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(b))
    opT = _as_operator(op, T)
    if adjoint is not None and not isinstance(adjoint, MIOperator):
        raise TypeError("expv_taylor_power: adjoint must be an MIOperator (A.adjoint())")
    ba, wa = _Arg(_host_view(b), T), _Arg(_host_view(w), T, writable=True)
    n = opT.shape[0]
    if int(np.prod(ba.shape)) != n:
        raise DimensionMismatch(f"length(b) [{int(np.prod(ba.shape))}] == size(A,1) [{n}] doesn't hold")
    if int(np.prod(wa.shape)) != n:
        raise DimensionMismatch(f"length(w) [{int(np.prod(wa.shape))}] == size(A,1) [{n}] doesn't hold")
    info, dinfo = (C.c_int64 * 12)(), (C.c_double * 12)()
    _check(L.load().expv_mi_expv_taylor_power(opT.ctx._h, opT._h, None if adjoint is None else adjoint._h, tr, ti, ba.ptr, ba.loc, wa.ptr,
                                              wa.loc, int(precision or 0), int(max_matvecs), info, dinfo), opT.ctx._h)
    wa.finish()
    d = dict(zip(_TAYLOR_POWER_INFO, (int(v) for v in info)))
    d.update(alpha=float(dinfo[0]), mu=complex(dinfo[1], dinfo[2]) if T.kind == "c" else float(dinfo[1]), normF=float(dinfo[3]),
             d=[float(v) for v in dinfo[4:12]])
    expv_taylor_power.last_info = d
    return (w, d) if return_info else w


def expv_taylor_power(t, A, b, *, adjoint=None, precision=None, max_matvecs=0, return_info=False, ctx=None):
    """exp(t A) b by the truncated Taylor series with the whole parameter search (see expv_taylor_power_): the result lives where
    ``b`` does and has the element type the device worked in."""
    op = _as_operator(A, None, ctx)
    T = _work_dtype(op.dtype, _np_dtype_of(b))
    if _is_torch(b) and not b.is_cuda:
        import torch
        w = torch.empty(b.shape[0], dtype=_torch_dtype(T))
    else:
        w = _empty_like(b, (b.shape[0],), T)
    return expv_taylor_power_(w, t, op, b, adjoint=adjoint, precision=precision, max_matvecs=max_matvecs, return_info=return_info, ctx=ctx)


def phiv_(w, t, Ks, k, *, correct=False, errest=False):
    """phiv!(w, t, Ks, k; correct, errest)  (krylov_phiv.jl:607-653)."""
    tr, ti, tc = _t_parts(t)
    wdt = _np_dtype_of(w)
    if (tc or Ks.T.kind == "c") and wdt.kind != "c":
        raise TypeError("InexactError: w must be complex when t or the basis is complex")
    wa = _Arg(w, _complex_of(Ks.T) if wdt.kind == "c" else _real_of(Ks.T), writable=True)
    if len(wa.shape) != 2 or wa.shape[0] != Ks.n + Ks.augmented or wa.shape[1] != k + 1:
        raise AssertionError("Dimension mismatch")
    err = C.c_double(0.0)
    _check(L.load().expv_mi_phiv_ks(Ks._h, tr, ti, int(k), int(bool(correct)), wa.ptr, wa.ld, wa.loc,
                                    _code(wa.dtype), C.byref(err)), Ks.ctx._h)
    wa.finish()
    return (w, err.value) if errest else w


def phiv(t, A, b, k=None, *, correct=False, errest=False, **kw):
    """phiv(t, A, b, k; correct, errest, kwargs...) and phiv(t, Ks, k; ...)  (krylov_phiv.jl:563-575)."""
    if isinstance(A, KrylovSubspace):
        Ks, kk = A, b
        w = np.empty((Ks.n, kk + 1), dtype=_complex_of(Ks.T) if _t_parts(t)[2] else Ks.T, order="F")
        return phiv_(w, t, Ks, kk, correct=correct, errest=errest)
    Ks = arnoldi(A, b, **kw)
    wdt = _complex_of(Ks.T) if _t_parts(t)[2] else Ks.T
    w = _empty_like(b, (b.shape[0], k + 1), wdt)
    res = phiv_(w, t, Ks, k, correct=correct, errest=errest)
    # result type of the reference: promote_type(typeof(t), eltype(A), eltype(b)) -- Float32 operands give a Float32 result
    rdt = _ref_dtype(_t_dtype(t), _src_dtype(A), _np_dtype_of(b))
    return (_round_to(res[0], rdt), res[1]) if errest else _round_to(res, rdt)


# ---------------------------------------------------------------------------------------------
# expv_timestep / phiv_timestep                           krylov_phiv_adaptive.jl:57-453
# ---------------------------------------------------------------------------------------------
class _TsCaches:
    def __init__(self, ctx, dtype, n, maxiter, p):
        h = C.c_void_p()
        _check(L.load().expv_mi_timestep_caches_create(ctx._h, _code(dtype), int(n), int(maxiter), int(p),
                                                       C.byref(h)), ctx._h)
        self._h, self.ctx = h, ctx
        self._finalizer = weakref.finalize(self, L.load().expv_mi_timestep_caches_destroy, h)


def timestep_caches(u_prototype, maxiter, p, ctx=None):
    """_phiv_timestep_caches(u_prototype, maxiter, p)  (krylov_phiv_adaptive.jl:502-511)."""
    return _TsCaches(ctx or default_context(), _work_dtype(_np_dtype_of(u_prototype)), u_prototype.shape[0],
                     maxiter, p)


def phiv_timestep_(U, ts, A, B, *, tau=0.0, m=None, tol=1e-7, opnorm=None, iop=0, correct=False, caches=None,
                   adaptive=False, delta=1.2, ishermitian=None, gamma=0.8, NA=0, verbose=False, ortho="auto",
                   out=None, stats=None, reuse_basis=True, keep_real=False):
    """phiv_timestep!(U, ts, A, B; ...)  (krylov_phiv_adaptive.jl:260-453).  ``ts`` is sorted in place.  ``keep_real=True``: a real
    operator meeting complex ``B`` / ``U`` of its precision is used as it is stored (expv_mi_phiv_timestep_realop)."""
    Bdt = _np_dtype_of(B)
    T = _work_dtype(Bdt)
    op = _as_operator_for(A, T, None, keep_real)
    mixed = bool(keep_real) and _is_mixed(op, T)
    if op.dtype != T and not mixed:
        T = _work_dtype(op.dtype, T)
    n = op.shape[0]
    Ba = _Arg(B, T)
    ncoef = Ba.shape[1] if len(Ba.shape) == 2 else 1
    Ua = _Arg(U, T, writable=True)
    nsnap = Ua.shape[1] if len(Ua.shape) == 2 else 1
    ts_arr = ts if isinstance(ts, np.ndarray) and ts.dtype == np.float64 and ts.flags.c_contiguous \
        else np.ascontiguousarray(ts, dtype=np.float64)
    if len(ts_arr) != nsnap:
        raise AssertionError("Dimension mismatch")
    if not (n == Ba.shape[0] == Ua.shape[0]):
        raise AssertionError("Dimension mismatch")
    o = L.TimestepOpts()
    L.load().expv_mi_timestep_opts_default(C.byref(o))
    o.tau, o.tol, o.delta, o.gamma = float(tau), float(tol), float(delta), float(gamma)
    if opnorm is not None:
        o.has_opnorm = 1
        o.opnorm = float(opnorm if np.isscalar(opnorm) else opnorm(A if not isinstance(A, MIOperator) else A.src,
                                                                   np.inf))
    o.m = int(m) if m is not None else 0
    o.iop, o.correct, o.adaptive = int(iop), int(bool(correct)), int(bool(adaptive))
    o.ishermitian = -1 if ishermitian is None else int(bool(ishermitian))
    o.verbose = int(bool(verbose))
    o.ortho = {"auto": 0, "mgs": 1, "lowsync": 2}[ortho] if isinstance(ortho, str) else int(ortho)
    o.NA = int(NA)
    o.no_basis_reuse = int(not reuse_basis)
    if verbose:
        sink = out if out is not None else print
    else:      # not verbose: the only line the library sends is its slow-progress notice (stats["stalled_steps"]) -- a warning
        import warnings
        sink = lambda line: warnings.warn(line, RuntimeWarning, stacklevel=3)
    cb = L.PRINT_FN(lambda line, user: sink(line.decode()))
    o.print = cb
    st = L.TimestepStats()
    entry = L.load().expv_mi_phiv_timestep_realop if mixed else L.load().expv_mi_phiv_timestep
    _check(entry(op.ctx._h, op._h, int(nsnap), ts_arr.ctypes.data_as(L._pd), Ba.ptr, Ba.ld,
                                          int(ncoef), Ba.loc, Ua.ptr, Ua.ld, Ua.loc, C.byref(o),
                                          caches._h if caches is not None else None, C.byref(st)), op.ctx._h)
    Ua.finish()
    if ts_arr is not ts and isinstance(ts, np.ndarray):
        ts[...] = ts_arr
    if stats is not None:
        stats.update(num_timesteps=st.num_timesteps, matvecs=st.matvecs, m=st.m_final, arnoldi_calls=st.arnoldi_calls,
                     arnoldi_reused=st.arnoldi_reused, stalled_steps=st.stalled_steps)
    return U


def phiv_timestep(ts, A, B, **kw):
    """phiv_timestep(ts, A, B; ...)  (krylov_phiv_adaptive.jl:184-191)."""
    op = _as_operator(A, None)
    T = _work_dtype(_np_dtype_of(B), op.dtype)
    n = op.shape[0]
    if np.isscalar(ts):
        u = _empty_like(B, (n,), T)
        return phiv_timestep_(u, np.array([float(ts)]), op, B, **kw)
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    U = _empty_like(B, (n, len(ts)), T)
    return phiv_timestep_(U, ts, op, B, **kw)


def expv_timestep(ts, A, b, **kw):
    """expv_timestep(ts, A, b; ...)  (krylov_phiv_adaptive.jl:57-67): the p = 0 case."""
    return phiv_timestep(ts, A, b, **kw)


def expv_timestep_(u, ts, A, b, **kw):
    """expv_timestep!(u, t, A, b; ...)  (krylov_phiv_adaptive.jl:99-114)."""
    if np.isscalar(ts):
        ts = np.array([float(ts)])
    return phiv_timestep_(u, ts, A, b, **kw)


# ---------------------------------------------------------------------------------------------
# kiops                                                                    kiops.jl:57-281
# ---------------------------------------------------------------------------------------------
def kiops(tau_out, A, u, *, mmin=10, mmax=128, m=None, tol=1e-7, opnorm=None, iop=2, ishermitian=None, task1=False,
          ortho="auto", allow_complex=False):
    """kiops(tau_out, A, u; mmin, mmax, m, tol, iop, ishermitian, task1) -> (w, stats).

    The reference is real-only (kiops.jl:89, arnoldi.jl:197-200).  ``allow_complex=True`` selects the
    mathematical extension this build defines for complex operands (no reference behaviour exists)."""
    op = _as_operator(A, None)
    udt = _np_dtype_of(u)
    T = _work64(op.dtype, udt)       # the reference method is Float64-only (kiops.jl:89: w = zeros(n, numSteps))
    if T.kind == "c" and not allow_complex:
        raise TypeError("kiops: complex operands have no method in the reference (kiops.jl:89, arnoldi.jl:197)")
    op = _as_operator(op, T)
    tau_nd = np.ndim(tau_out)
    tau_arr = np.atleast_1d(np.asarray(tau_out, dtype=np.float64)).ravel(order="F").copy()
    tau_ncols = 1 if tau_nd < 2 else np.shape(tau_out)[1]
    ua = _Arg(u, T)
    ncols_u = ua.shape[1] if len(ua.shape) == 2 else 1
    n = op.shape[0]
    if ua.shape[0] != n:
        raise DimensionMismatch("size(u,1) == size(A,1) doesn't hold")
    w = _empty_like(u, (n, 1), T)
    wa = _Arg(w, T, writable=True)
    o = L.KiopsOpts()
    L.load().expv_mi_kiops_opts_default(C.byref(o))
    o.mmin, o.mmax, o.iop, o.task1 = int(mmin), int(mmax), int(iop), int(bool(task1))
    o.m = int(m) if m is not None else 0
    o.tol = float(tol)
    o.ishermitian = -1 if ishermitian is None else int(bool(ishermitian))
    o.ortho = {"auto": 0, "mgs": 1, "lowsync": 2}[ortho] if isinstance(ortho, str) else int(ortho)
    st = (C.c_int64 * 5)()
    _check(L.load().expv_mi_kiops(op.ctx._h, op._h, tau_arr.ctypes.data_as(L._pd), int(tau_arr.size), int(tau_ncols),
                                  ua.ptr, ua.ld, int(ncols_u), ua.loc, wa.ptr, wa.ld, wa.loc, C.byref(o), st),
           op.ctx._h)
    wa.finish()
    return w, tuple(int(x) for x in st)


# ---------------------------------------------------------------------------------------------
# batch of independent problems (BASELINE config 5)
# ---------------------------------------------------------------------------------------------
def expv_batch(ts, pattern, vals, B, *, m=None, tol=1e-7, iop=0, ishermitian=False, ctx=None, return_m=False):
    """W[:, p] = expv(ts[p], A_p, B[:, p]; m, tol, iop, ishermitian) for nprob operators A_p that share
    the sparsity pattern of the scipy matrix ``pattern`` (CSR order) and have values ``vals[p, :]``.

    Equivalent to a host loop over the reference's ``expv`` (the reference has no batching); all problems
    advance in lock step inside the library.  ``vals``/``B`` may be numpy arrays or torch CUDA tensors
    (B as an (n, nprob) column-major view, e.g. ``torch.empty(nprob, n).t()``)."""
    ctx = ctx or default_context()
    P = pattern.tocsr()
    P.sort_indices()
    n = P.shape[0]
    nnz = int(P.nnz)
    vdt, bdt = _np_dtype_of(vals), _np_dtype_of(B)
    T = _work_dtype(vdt, bdt)          # every BlasFloat: Float32 / ComplexF32 batches are computed on 32-bit storage
    class _Raw:          # problem-major (nprob, nnz) values: row-major is the wanted layout here
        pass
    va = _Raw()
    if _is_torch(vals):
        import torch
        vt = vals.to(_torch_dtype(T)).contiguous()
        if not vt.is_cuda:
            raise TypeError("torch tensors must live on the GPU (or pass a numpy array)")
        va.ptr, va.loc, va.keep, nprob = vt.data_ptr(), L.DEVICE, vt, int(vt.shape[0])
        if vt.numel() != nprob * nnz:
            raise DimensionMismatch("vals must hold nprob x nnz values")
    else:
        vh = np.ascontiguousarray(np.asarray(vals, dtype=T))
        nprob = int(vh.shape[0])
        if vh.size != nprob * nnz:
            raise DimensionMismatch("vals must hold nprob x nnz values")
        va.ptr, va.loc, va.keep = vh.ctypes.data, L.HOST, vh
    Ba = _Arg(B, T)
    if Ba.shape[0] != n or (len(Ba.shape) == 2 and Ba.shape[1] != nprob):
        raise DimensionMismatch("B must be n x nprob")
    W = _empty_like(B, (n, nprob), T)
    Wa = _Arg(W, T, writable=True)
    rp = np.ascontiguousarray(P.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(P.indices, dtype=np.int32)
    tarr = np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (nprob,)))
    o = _opts(m, tol, iop, 0, ishermitian, "auto")
    mu = np.zeros(nprob, dtype=np.int32)
    _check(L.load().expv_mi_expv_batch(ctx._h, _code(T), n, int(nprob), rp.ctypes.data, ci.ctypes.data, va.ptr, nnz,
                                       L.HOST if va.loc == L.HOST else L.DEVICE, tarr.ctypes.data_as(L._pd), Ba.ptr, Ba.ld,
                                       Ba.loc, Wa.ptr, Wa.ld, Wa.loc, C.byref(o), mu.ctypes.data_as(C.POINTER(C.c_int32))),
           ctx._h)
    Wa.finish()
    return (W, mu) if return_m else W


def expv_batch_multi(ts, pattern, vals, B, ctxs, *, m=None, tol=1e-7, iop=0, ishermitian=False, return_m=False, out=None):
    """The same batch sharded over several contexts (one per GPU) from ONE host process -- expv_mi_expv_batch_multi: what
    a Julia host calls for BASELINE config 5.  ``vals`` / ``B`` are host arrays; the result is a host matrix, or -- when
    ``out`` is a DeviceArray / torch tensor on ctxs[0]'s device -- gathered there by peer copies."""
    P = pattern.tocsr()
    P.sort_indices()
    n, nnz = P.shape[0], int(P.nnz)
    T = _work_dtype(_np_dtype_of(vals), _np_dtype_of(B))
    vh = np.ascontiguousarray(np.asarray(vals, dtype=T))
    nprob = int(vh.shape[0])
    if vh.size != nprob * nnz:
        raise DimensionMismatch("vals must hold nprob x nnz values")
    Ba = _Arg(np.asarray(B), T)
    if Ba.shape[0] != n or (len(Ba.shape) == 2 and Ba.shape[1] != nprob):
        raise DimensionMismatch("B must be n x nprob")
    W = out if out is not None else np.empty((n, nprob), dtype=T, order="F")
    Wa = _Arg(W, T, writable=True)
    rp = np.ascontiguousarray(P.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(P.indices, dtype=np.int32)
    tarr = np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (nprob,)))
    o = _opts(m, tol, iop, 0, ishermitian, "auto")
    mu = np.zeros(nprob, dtype=np.int32)
    hs = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    code = L.load().expv_mi_expv_batch_multi(hs, len(ctxs), _code(T), n, nprob, rp.ctypes.data, ci.ctypes.data, vh.ctypes.data, nnz,
                                             tarr.ctypes.data_as(L._pd), Ba.ptr, Ba.ld, Wa.ptr, Wa.ld, Wa.loc, C.byref(o),
                                             mu.ctypes.data_as(C.POINTER(C.c_int32)))
    if code != 0:
        for c in ctxs:            # the failing shard's context holds the message
            msg = L.load().expv_mi_last_error(c._h)
            if msg:
                _check(code, c._h)
        _check(code, ctxs[0]._h)
    Wa.finish()
    return (W, mu) if return_m else W


# ---------------------------------------------------------------------------------------------
# host small-dense functions (no GPU needed)
# ---------------------------------------------------------------------------------------------
_HOST_CODES = {np.dtype(np.float64): L.F64, np.dtype(np.complex128): L.C64, np.dtype(np.float32): L.F32,
               np.dtype(np.complex64): L.C32}


# ------------------------------------------------------------------------------------------
# final gather over RCCL through the C ABI (include/expv_mi.h: expv_mi_comm_create / expv_mi_gather_rccl) -- the form a host
# without torch.distributed uses; dist.py keeps the torch.distributed form beside it
# ------------------------------------------------------------------------------------------
def rccl_available():
    return bool(L.load().expv_mi_rccl_available())


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId: rank 0 makes them, the host hands them to the other ranks."""
    buf = C.create_string_buffer(128)
    _check(L.load().expv_mi_rccl_unique_id(buf))
    return buf.raw


class RcclComm:
    """An RCCL communicator bound to a context (collective constructor: every rank calls it with the same id)."""

    def __init__(self, ctx, unique_id, nranks, rank):
        if len(unique_id) != 128:
            raise ValueError("unique_id: 128 bytes (rccl_unique_id())")
        self.ctx, self.nranks, self.rank = ctx, int(nranks), int(rank)
        h = C.c_void_p()
        idb = C.create_string_buffer(bytes(unique_id), 128)
        _check(L.load().expv_mi_comm_create(ctx._h, idb, self.nranks, self.rank, C.byref(h)), ctx._h)
        self._h = h
        self._finalizer = weakref.finalize(self, L.load().expv_mi_comm_destroy, h)

    def all_gather(self, send, out=None):
        """recv[r * count : (r + 1) * count] = rank r's `send` (device tensors; enqueued on the context's stream)."""
        import torch
        dt = _np_dtype_of(send)
        if not send.is_contiguous():
            raise ValueError("all_gather: contiguous send block")
        count = send.numel()
        if out is None:
            out = torch.empty(self.nranks * count, dtype=send.dtype, device=send.device)
        _check(L.load().expv_mi_gather_rccl(self._h, C.c_void_p(send.data_ptr()), C.c_void_p(out.data_ptr()), count, _code(dt)), self.ctx._h)
        return out

    def all_gather_raw(self, send_ptr, recv_ptr, count, dtype):
        """The same on raw device pointers (DeviceArray.ptr): `count` elements of `dtype` per rank."""
        _check(L.load().expv_mi_gather_rccl(self._h, C.c_void_p(int(send_ptr)), C.c_void_p(int(recv_ptr)), int(count), _code(np.dtype(dtype))), self.ctx._h)

    def destroy(self):
        if self._finalizer.alive:
            self._finalizer()


# ---------------------------------------------------------------------------------------------
# dense matrices on the device: exponential!(A) for a GPU array (exp.jl:56-58), mul!(C, A, B, alpha, beta)
# ---------------------------------------------------------------------------------------------
_DENSE_KINDS = "float32 / float64 / complex64 / complex128"


def _dense_np_dtype(x):
    """element type of a dense matrix argument; TypeError for anything but the four BlasFloats (integers included)"""
    if isinstance(x, DeviceArray):
        dt = x.dtype
    elif _is_torch(x):
        import torch
        dt = {torch.float64: np.dtype(np.float64), torch.complex128: np.dtype(np.complex128),
              torch.float32: np.dtype(np.float32), torch.complex64: np.dtype(np.complex64)}.get(x.dtype)
        if dt is None:
            raise TypeError(f"dense matrix entries must be {_DENSE_KINDS}, not {x.dtype}")
        return dt
    else:
        dt = np.asarray(x).dtype
    if dt not in _HOST_CODES:
        raise TypeError(f"dense matrix entries must be {_DENSE_KINDS}, not {dt}")
    return np.dtype(dt)


def _square(shape, what):
    if len(shape) != 2 or shape[0] != shape[1]:
        raise DimensionMismatch(f"{what}: matrix is not square: dimensions are {tuple(shape)}")
    return int(shape[0])


_EXPM_INFO = ("order", "squarings", "row_exchanges", "microseconds")
_EXPM_BALANCE_INFO = _EXPM_INFO + ("ilo", "ihi", "sweeps", "balance_microseconds")


def exponential_(A, balance=False, ctx=None, return_info=False):
    """exponential!(A) for a dense matrix, computed on the device whatever its size (exp.jl:56-58 -> ExpMethodHigham2005(false),
    no balancing; expv_mi_expm).  balance=True: exponential!(A, ExpMethodHigham2005Base()) -- gebal first, the norm taken after
    it, unbalance at the end (expv_mi_expm_balanced): the one to take for badly scaled matrices.  A: a 2-D torch tensor on the
    GPU or a DeviceArray (used in place) or a numpy array (staged through HBM, result copied back).  Row-major (C-contiguous)
    storage is passed as it is -- exp(A') = exp(A)' --, column-major storage with its own leading dimension, any other stride
    pattern through a copy.  Returns A (and, with return_info, a dict: Pade order, squarings, row exchanges of the LU,
    microseconds; with balance also ilo, ihi, sweeps of the scaling loop and the microseconds of balancing)."""
    dt = _dense_np_dtype(A)
    shape = tuple(A.shape)
    n = _square(shape, "exponential!")
    info = (C.c_int64 * 8)()

    def run(c, ptr, lda, loc):
        fn = L.load().expv_mi_expm_balanced if balance else L.load().expv_mi_expm
        _check(fn(c._h, _code(dt), n, ptr, max(int(lda), n, 1), loc, info), c._h)

    if isinstance(A, DeviceArray):
        run(ctx or A.ctx, A.ptr, n, L.DEVICE)
    elif _is_torch(A):
        if not A.is_cuda:
            raise TypeError("torch tensors must live on the GPU (or pass a numpy array)")
        c = ctx or default_context()
        if n > 0:
            if n == 1 or (A.stride(1) == 1 and A.stride(0) >= n):         # row-major: the transpose, column-major
                _torch_ready(A)
                run(c, A.data_ptr(), A.stride(0) if n > 1 else 1, L.DEVICE)
            elif A.stride(0) == 1 and A.stride(1) >= n:
                _torch_ready(A)
                run(c, A.data_ptr(), A.stride(1), L.DEVICE)
            else:
                tmp = A.contiguous()
                _torch_ready(tmp)
                run(c, tmp.data_ptr(), n, L.DEVICE)
                A.copy_(tmp)
    else:
        if not isinstance(A, np.ndarray):
            raise TypeError("exponential_ works in place: pass a numpy array, a torch GPU tensor or a DeviceArray")
        c = ctx or default_context()
        if n > 0:
            if (A.flags.f_contiguous or A.flags.c_contiguous) and A.flags.writeable:
                run(c, A.ctypes.data, n, L.HOST)
            else:
                tmp = np.array(A, order="F", copy=True)
                run(c, tmp.ctypes.data, n, L.HOST)
                A[...] = tmp
    if return_info:
        names = _EXPM_BALANCE_INFO if balance else _EXPM_INFO
        return A, dict(zip(names, (int(v) for v in info[:len(names)])))
    return A


def exponential(A, balance=False, ctx=None, return_info=False):
    """exponential(A): a new array of A's kind holding exp(A) (see exponential_)."""
    _dense_np_dtype(A)
    if isinstance(A, DeviceArray):
        B = DeviceArray.from_host(A.to_host(), A.ctx)
    elif _is_torch(A):
        B = A.clone()
    else:
        B = np.array(A, order="F", copy=True)
    return exponential_(B, balance=balance, ctx=ctx, return_info=return_info)


def balance_(A, ctx=None):
    """LAPACK.gebal!('B', A) for a dense matrix, computed on the device (expv_mi_gebal): A is balanced in place -- a 2-D torch
    tensor on the GPU, a DeviceArray or a numpy array (staged through HBM).  Balancing is not symmetric in A and A', so storage that
    is not column-major goes through a column-major copy.  Returns (ilo, ihi, scale): 1-based bounds and LAPACK's scale vector
    (float64: the factors inside ilo..ihi, the exchanged positions outside)."""
    dt = _dense_np_dtype(A)
    n = _square(tuple(A.shape), "balance!")
    ilo, ihi = C.c_int64(1), C.c_int64(0)
    scale = np.ones(n, dtype=np.float64)

    def run(c, ptr, lda, loc):
        _check(L.load().expv_mi_gebal(c._h, _code(dt), n, ptr, max(int(lda), n, 1), loc, C.byref(ilo), C.byref(ihi), scale.ctypes.data), c._h)

    if isinstance(A, DeviceArray):
        run(ctx or A.ctx, A.ptr, n, L.DEVICE)
    elif _is_torch(A):
        if not A.is_cuda:
            raise TypeError("torch tensors must live on the GPU (or pass a numpy array)")
        c = ctx or default_context()
        if n > 0:
            if n == 1 or (A.stride(0) == 1 and A.stride(1) >= n):
                _torch_ready(A)
                run(c, A.data_ptr(), A.stride(1) if n > 1 else 1, L.DEVICE)
            else:
                tmp = A.t().contiguous()          # the rows of tmp are the columns of A
                _torch_ready(tmp)
                run(c, tmp.data_ptr(), n, L.DEVICE)
                if getattr(c, "_async_outputs", False):
                    c.sync()
                A.copy_(tmp.t())
    else:
        if not isinstance(A, np.ndarray):
            raise TypeError("balance_ works in place: pass a numpy array, a torch GPU tensor or a DeviceArray")
        c = ctx or default_context()
        if n > 0:
            if A.flags.f_contiguous and A.flags.writeable:
                run(c, A.ctypes.data, n, L.HOST)
            else:
                tmp = np.array(A, order="F", copy=True)
                run(c, tmp.ctypes.data, n, L.HOST)
                A[...] = tmp
    return int(ilo.value), int(ihi.value), scale


PHI_MAX_K = 16
_PHI_INFO = ("degree", "scalings", "products", "microseconds")


def _device_view(base, offset, shape):
    """a DeviceArray over part of another one's storage (the parent is kept alive)"""
    v = DeviceArray.__new__(DeviceArray)
    v.ctx, v.shape, v.dtype, v._base = base.ctx, tuple(shape), base.dtype, base
    v.nbytes = int(np.prod(v.shape)) * v.dtype.itemsize
    v.ptr = base.ptr + int(offset)
    return v


def _dense_kind(x):
    return "device" if isinstance(x, DeviceArray) else "torch" if _is_torch(x) else "numpy" if isinstance(x, np.ndarray) else None


def _phi_order(k, what):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= PHI_MAX_K:
        raise ValueError(f"{what}: k must be an integer in 0..{PHI_MAX_K}, not {k!r}")
    return int(k)


def _phi_blocks(out, n, k, dt, ka):
    """`out` of phi! as a list of k + 1 n x n matrices: a sequence of them, or the blocks of one n x (k + 1) n slab"""
    if isinstance(out, (list, tuple)):
        blocks = list(out)
        if len(blocks) != k + 1:
            raise DimensionMismatch(f"phi!: out has {len(blocks)} matrices, k + 1 = {k + 1}")
    else:
        if tuple(out.shape) != (n, (k + 1) * n):
            raise DimensionMismatch(f"phi!: out is {tuple(out.shape)}, need {k + 1} matrices or one {(n, (k + 1) * n)} slab")
        if isinstance(out, DeviceArray):
            blocks = [_device_view(out, j * n * n * out.dtype.itemsize, (n, n)) for j in range(k + 1)]
        else:
            blocks = [out[:, j * n:(j + 1) * n] for j in range(k + 1)]
    for b in blocks:
        if _dense_kind(b) != ka or (ka == "torch" and not b.is_cuda):
            raise TypeError("phi!: out and A must be of one kind (numpy arrays, torch GPU tensors or DeviceArrays)")
        if tuple(b.shape) != (n, n):
            raise DimensionMismatch(f"phi!: an output matrix is {tuple(b.shape)}, A is {(n, n)}")
        if _dense_np_dtype(b) != dt:
            raise TypeError(f"phi!: out must have A's element type {dt}")
    return blocks


def _mat_layout(x, n):
    """(pointer, leading dimension, "col" / "row") of an n x n numpy array or torch tensor in one of the two plain layouts, else None"""
    if _is_torch(x):
        s0, s1, ptr = x.stride(0), x.stride(1), x.data_ptr()
    else:
        if x.strides[0] % x.itemsize or x.strides[1] % x.itemsize:
            return None
        s0, s1, ptr = x.strides[0] // x.itemsize, x.strides[1] // x.itemsize, x.ctypes.data
    if n <= 1:
        return ptr, 1, "any"
    if s0 == 1 and s1 >= n:
        return ptr, s1, "col"
    if s1 == 1 and s0 >= n:
        return ptr, s0, "row"
    return None


def phi_(out, A, k, ctx=None, return_info=False):
    """phi!(out, A, k) for a dense matrix, computed on the device (phi.jl:159-257; expv_mi_phi: scaling and recovering with a Taylor
    core): out[j] <- phi_j(A), j = 0 .. k <= 16, A unchanged.  A: a 2-D torch tensor on the GPU, a DeviceArray or a numpy array
    (staged through HBM); out: a sequence of k + 1 matrices of A's kind and element type, or one n x (k + 1) n slab whose blocks
    they are.  Column-major storage is used in place; so is row-major storage when A and every out[j] have it -- phi_j(A') =
    phi_j(A)' --; mixed or strided layouts go through a copy.  Returns out (and, with return_info, a dict: Taylor degree, scalings,
    products, microseconds).  A non-finite entry raises ArgumentError and leaves out as it was."""
    dt = _dense_np_dtype(A)
    n = _square(tuple(A.shape), "phi!")
    k = _phi_order(k, "phi!")
    ka = _dense_kind(A)
    if ka is None:
        raise TypeError("phi!: pass a numpy array, a torch GPU tensor or a DeviceArray")
    if ka == "torch" and not A.is_cuda:
        raise TypeError("torch tensors must live on the GPU (or pass a numpy array)")
    blocks = _phi_blocks(out, n, k, dt, ka)
    info = (C.c_int64 * 8)()

    def run(c, a_ptr, lda, ptrs, ldo, loc):
        arr = (C.c_void_p * (k + 1))(*[int(p) for p in ptrs])
        _check(L.load().expv_mi_phi(c._h, _code(dt), n, k, a_ptr, max(int(lda), n, 1), arr, max(int(ldo), n, 1), loc, info), c._h)

    if n > 0:
        if ka == "device":
            run(ctx or A.ctx, A.ptr, n, [b.ptr for b in blocks], n, L.DEVICE)
        else:
            is_t = ka == "torch"
            c = ctx or default_context()
            loc = L.DEVICE if is_t else L.HOST
            if not is_t and not all(b.flags.writeable for b in blocks):
                raise ValueError("phi!: an output array is read-only")
            lay = [_mat_layout(x, n) for x in [A] + blocks]
            orient = {l[2] for l in lay if l is not None} - {"any"}
            if all(l is not None for l in lay) and len(orient) <= 1 and len({l[1] for l in lay[1:]}) == 1:
                if is_t:
                    _torch_ready(A, *blocks)
                run(c, lay[0][0], lay[0][1], [l[0] for l in lay[1:]], lay[1][1], loc)
            elif is_t:          # row-major copies: the transposed problem, column-major
                import torch
                a = A.contiguous()
                tmp = torch.empty((k + 1, n, n), dtype=A.dtype, device=A.device)
                _torch_ready(a, tmp)
                run(c, a.data_ptr(), n, [tmp[j].data_ptr() for j in range(k + 1)], n, loc)
                for j, b in enumerate(blocks):
                    b.copy_(tmp[j])
            else:
                a = np.asfortranarray(A)
                tmp = np.empty((n, (k + 1) * n), dtype=dt, order="F")
                run(c, a.ctypes.data, n, [tmp.ctypes.data + j * n * n * dt.itemsize for j in range(k + 1)], n, loc)
                for j, b in enumerate(blocks):
                    b[...] = tmp[:, j * n:(j + 1) * n]
    if return_info:
        return out, dict(zip(_PHI_INFO, (int(v) for v in info[:4])))
    return out


def phi(A, k, ctx=None, return_info=False):
    """phi(A, k): [phi_0(A), ..., phi_k(A)] as the block views of one new n x (k + 1) n slab of A's kind (see phi_)."""
    dt = _dense_np_dtype(A)
    n = _square(tuple(A.shape), "phi")
    k = _phi_order(k, "phi")
    if isinstance(A, DeviceArray):
        slab = DeviceArray((n, (k + 1) * n), dt, ctx or A.ctx)
        blocks = [_device_view(slab, j * n * n * dt.itemsize, (n, n)) for j in range(k + 1)]
    elif _is_torch(A):
        import torch
        if not A.is_cuda:
            raise TypeError("torch tensors must live on the GPU (or pass a numpy array)")
        if n > 1 and A.stride(0) == 1:        # column-major A: a column-major slab
            slab = torch.empty(((k + 1) * n, n), dtype=A.dtype, device=A.device).t()
        else:
            slab = torch.empty((n, (k + 1) * n), dtype=A.dtype, device=A.device)
        blocks = [slab[:, j * n:(j + 1) * n] for j in range(k + 1)]
    else:
        if not isinstance(A, np.ndarray):
            raise TypeError("phi: pass a numpy array, a torch GPU tensor or a DeviceArray")
        slab = np.empty((n, (k + 1) * n), dtype=dt, order="C" if (n > 1 and A.flags.c_contiguous) else "F")
        blocks = [slab[:, j * n:(j + 1) * n] for j in range(k + 1)]
    res = phi_(blocks, A, k, ctx=ctx, return_info=return_info)
    return (blocks, res[1]) if return_info else blocks


def _dense_dev_arg(x, dt, what):
    """(pointer, leading dimension, shape) of a column-major device matrix"""
    if isinstance(x, DeviceArray):
        if x.dtype != dt or x.ndim != 2:
            raise TypeError(f"mul_: {what} must be a 2-D device array of dtype {dt}")
        return x.ptr, max(x.shape[0], 1), x.shape, x
    if not (_is_torch(x) and x.is_cuda):
        raise TypeError(f"mul_: {what} must be a torch tensor on the GPU or a DeviceArray")
    if x.dim() != 2 or _dense_np_dtype(x) != dt:
        raise TypeError(f"mul_: {what} must be a 2-D tensor of dtype {dt}")
    return None, None, tuple(x.shape), x


def mul_(Cm, A, B, alpha=1, beta=0, ctx=None):
    """mul!(C, A, B, alpha, beta): C = alpha A B + beta C for matrices on the device, on the matrix cores (expv_mi_gemm).  torch
    tensors in column-major storage (e.g. torch.empty(n, m).t()) are used in place; row-major A / B are copied, a row-major C is
    refused.  C must not alias A or B."""
    dt = _dense_np_dtype(Cm)
    args = [_dense_dev_arg(x, dt, w) for x, w in ((Cm, "C"), (A, "A"), (B, "B"))]
    (m, n), (ma, k), (kb, nb) = (tuple(int(v) for v in a[2]) for a in args)
    if ma != m or kb != k or nb != n:
        raise DimensionMismatch(f"mul!: C is {m}x{n}, A is {ma}x{k}, B is {kb}x{nb}")
    alpha, beta = complex(alpha), complex(beta)
    if dt.kind != "c" and (alpha.imag != 0 or beta.imag != 0):
        raise TypeError("InexactError: complex scalar with a real element type")
    ptrs, keep = [], []
    for i, (ptr, ld, shape, x) in enumerate(args):
        if ptr is None:
            if not (x.stride(0) == 1 and (shape[1] <= 1 or x.stride(1) >= max(shape[0], 1))) and min(shape) > 0:
                if i == 0:
                    raise TypeError("output matrix must be column-major (e.g. torch.empty(n, m).t())")
                x = x.t().contiguous().t()
            keep.append(x)
            ptr, ld = x.data_ptr(), (x.stride(1) if shape[1] > 1 else max(shape[0], 1))
        ptrs.append((ptr, max(int(ld), 1)))
    tens = [x for x in keep if _is_torch(x)]
    if tens:
        _torch_ready(*tens)
    c = ctx or (Cm.ctx if isinstance(Cm, DeviceArray) else default_context())
    _check(L.load().expv_mi_gemm(c._h, _code(dt), m, n, k, alpha.real, alpha.imag, ptrs[1][0], ptrs[1][1], ptrs[2][0], ptrs[2][1],
                                 beta.real, beta.imag, ptrs[0][0], ptrs[0][1]), c._h)
    if not getattr(c, "_async_outputs", False):      # stream-ordered on the library's stream: torch reads C on its own
        c.sync()
    return Cm


def _host_dtype(*dts):
    """Element type of the host small-dense functions: every BlasFloat is kept (Float32 stays Float32)."""
    dt = np.result_type(*[np.dtype(d) for d in dts])
    if dt.kind not in "fc" or dt.itemsize < 4:
        dt = np.result_type(dt, np.float64)
    if dt.itemsize > 16 or (dt.kind == "f" and dt.itemsize > 8):
        dt = np.dtype(np.complex128 if dt.kind == "c" else np.float64)
    if dt == np.dtype(np.float16):
        dt = np.dtype(np.float32)
    return dt


def host_expm(A):
    """exponential!(copy(A), ExpMethodHigham2005Base()) on the host (exp_baseexp.jl:112-161), for every BlasFloat element
    type (Float32 / ComplexF32 stay what they are: test/basictests.jl:952-974)."""
    A = np.array(A, dtype=_host_dtype(np.asarray(A).dtype), order="F", copy=True)
    n = A.shape[0]
    _check(L.load().expv_mi_host_expm(_HOST_CODES[A.dtype], n, A.ctypes.data, max(n, 1)))
    return A


def host_gebal(A):
    """LAPACK.gebal!('B', copy(A)) by the host routine behind host_expm (xGEBAL job 'B', in A's own element type; no GPU):
    returns (balanced copy, ilo, ihi, scale)."""
    A = np.array(A, dtype=_host_dtype(np.asarray(A).dtype), order="F", copy=True)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise DimensionMismatch(f"host_gebal: matrix is not square: dimensions are {A.shape}")
    n = A.shape[0]
    ilo, ihi = C.c_int64(1), C.c_int64(0)
    scale = np.ones(n, dtype=np.float64)
    _check(L.load().expv_mi_host_gebal(_HOST_CODES[A.dtype], n, A.ctypes.data, max(n, 1), C.byref(ilo), C.byref(ihi), scale.ctypes.data))
    return A, int(ilo.value), int(ihi.value), scale


def host_pattern_info(A, dtype=np.float64):
    """Which storage forms a sparse pattern gets and hence which factorisation path it takes (host only; no reference
    counterpart).  A: scipy sparse matrix (converted to CSR)."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(A.indices, dtype=np.int32)
    out = np.zeros(8, dtype=np.int64)
    _check(L.load().expv_mi_host_pattern_info(n, rp.ctypes.data, ci.ctypes.data, _code(np.dtype(dtype)), out.ctypes.data))
    info = {"sell": bool(out[0]), "bandwidth": int(out[1]), "pipeline_dia_diagonals": int(out[2]),
            "general_dia_diagonals": int(out[3]), "general_dia_max_offset": int(out[4]), "sell_wave_reach": int(out[5]),
            "rows_sorted_unique": bool(out[6]), "sell_cut": int(out[7])}
    if not info["sell"]:
        info["path"] = "modular (empty operator)"
    elif info["sell_cut"] > 0:
        info["path"] = "two-kernel step, SELL slots up to the cut + overflow pass (irregular rows)"
    elif info["pipeline_dia_diagonals"] or (np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.float32)) and info["bandwidth"] <= 8):
        info["path"] = "pipeline, halo form"
    elif np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.float32)) and (info["general_dia_diagonals"] or info["sell_wave_reach"] >= 0):
        info["path"] = ("pipeline, wave form (when the reach is small against the resident grid), else two-kernel step; a 2-D grid "
                        "stencil: pipeline, patch form under context option patch (host_patch_order)")
    else:
        info["path"] = "two-kernel step"
    return info


def host_dia_pattern(offsets, n, ld=None, align="col", arrays=True):
    """The scalar CSR pattern ``MIOperator.from_dia`` makes of stored diagonals and the creator's host-side checks (host only,
    expv_mi_host_dia_pattern): ``nnz``, the ``diagonals`` with |k| < n and their smallest / largest offset, and with ``arrays``
    ``rowptr``, ``colind`` and ``src`` -- the element index into ``data`` (rows of ``ld`` elements, default n) that each position
    reads.  Raises what the creator would raise."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, ld = int(n), int(n if ld is None else ld)
    lib = L.load()
    out = np.zeros(4, dtype=np.int64)
    op = offsets.ctypes.data if offsets.size else None
    _check(lib.expv_mi_host_dia_pattern(n, int(offsets.size), op, ld, _DIA_ALIGN[align], None, None, None, out.ctypes.data))
    info = {"nnz": int(out[0]), "diagonals": int(out[1]), "min_offset": int(out[2]), "max_offset": int(out[3])}
    if arrays:
        rp, ci, src = np.zeros(n + 1, dtype=np.int32), np.zeros(info["nnz"], dtype=np.int32), np.zeros(info["nnz"], dtype=np.int64)
        _check(lib.expv_mi_host_dia_pattern(n, int(offsets.size), op, ld, _DIA_ALIGN[align], rp.ctypes.data,
                                            ci.ctypes.data if ci.size else None, src.ctypes.data if src.size else None, out.ctypes.data))
        info.update(rowptr=rp, colind=ci, src=src)
    return info


def host_rcm(A, dtype=np.float64):
    """The bandwidth-reducing ordering operator creation computes for a pattern (reverse Cuthill-McKee on A + A'; host only, no
    reference counterpart): perm with perm[i] = the row that becomes row i, and what it does to the bandwidth / the step form."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(A.indices, dtype=np.int32)
    perm = np.zeros(n, dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    _check(L.load().expv_mi_host_rcm(n, rp.ctypes.data, ci.ctypes.data, _code(np.dtype(dtype)), perm.ctypes.data, out.ctypes.data))
    names = {3: "single-pass step, halo form", 2: "single-pass step, wave form", 1: "two-kernel step", 0: "two-kernel step + overflow pass"}
    return perm, {"bandwidth_before": int(out[0]), "bandwidth_after": int(out[1]), "form_before": names[int(out[2]) & 255],
                  "form_after": names[int(out[3])], "would_reorder": bool(int(out[2]) & 256)}


def host_patch_order(A, dtype=np.float64, mesh=False):
    """The grid-patch ordering operator creation would store a 2-D grid stencil in under context option ``patch`` (host only, no
    reference counterpart): (perm, ring_count per tile, info) -- perm is None when no 2-D grid is recognised in the pattern."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(A.indices, dtype=np.int32)
    perm = np.zeros(n, dtype=np.int32)
    tr = (16 // np.dtype(dtype).itemsize) * 256
    cnt = np.zeros((n + tr - 1) // tr, dtype=np.int32)
    out = np.zeros(8, dtype=np.int64)
    f = L.load().expv_mi_host_mesh_patch_order if mesh else L.load().expv_mi_host_patch_order      # mesh: patches of a mesh in any numbering
    _check(f(n, rp.ctypes.data, ci.ctypes.data, _code(np.dtype(dtype)), perm.ctypes.data, cnt.ctypes.data, out.ctypes.data))
    info = {"patch_form": bool(out[0]), "grid_row_length": int(out[1]), "tiles": int(out[2]), "longest_ring": int(out[3]),
            "mean_ring": (float(out[4]) / int(out[2])) if out[2] else 0.0, "tiles_ring_over_128": int(out[5]),
            "column_indices_stored": int(out[6]), "ring_entries_per_tile": int(out[7])}
    return (perm if out[0] else None), cnt, info


def host_phiv_dense(A, v, k):
    """phiv_dense(A, v, k)  (phi.jl:75-115), element type kept (see host_expm)."""
    dt = _host_dtype(np.asarray(A).dtype, np.asarray(v).dtype)
    A = np.asfortranarray(A, dtype=dt)
    v = np.ascontiguousarray(v, dtype=dt)
    m = A.shape[0]
    w = np.empty((m, k + 1), dtype=dt, order="F")
    _check(L.load().expv_mi_host_phiv_dense(_HOST_CODES[dt], m, int(k), A.ctypes.data, max(m, 1), v.ctypes.data,
                                            w.ctypes.data))
    return w


def host_symtridiag_exp_last(d, e, t):
    """last entry of host_symtridiag_expcol, computed from the first and last eigenvector rows only (O(n^2))."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    out = np.empty(1, dtype=np.complex128)
    tr, ti, _ = _t_parts(t)
    _check(L.load().expv_mi_host_symtridiag_exp_last(d.size, d.ctypes.data_as(L._pd), e.ctypes.data_as(L._pd), tr, ti,
                                                     out.ctypes.data_as(L._pd)))
    return complex(out[0])


def host_symtridiag_expcol(d, e, t):
    """Z*(exp.(t*lambda).*Z[1,:]) for SymTridiagonal(d, e)  (krylov_phiv.jl:227-228)."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    n = d.size
    out = np.empty(n, dtype=np.complex128)
    tr, ti, _ = _t_parts(t)
    _check(L.load().expv_mi_host_symtridiag_expcol(n, d.ctypes.data_as(L._pd), e.ctypes.data_as(L._pd), tr, ti,
                                                   out.ctypes.data_as(L._pd)))
    return out
