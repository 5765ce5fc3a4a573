"""Shared inputs of the caller-stream tests (tests/test_gpu_caller_stream.py on the device, tests/test_caller_stream_cpu.py on the host)
and the delay helper.  Nothing here needs a GPU to be imported; torch is imported inside the functions that use it.

Two kinds of things:

* operator / vector builders at the smallest sizes at which the step form in question is still selected: sparse operators of N = 4100
  rows (a few tiles of 4096 / sizeof(element) rows and a ragged tail, the size tests/test_gpu_limits.py uses), dense ones of 96 and 130;
* LATE: the cases of "an input produced earlier on the caller's stream".  Each has a decoy input x[0] (valid, never zero: a zero vector
  takes the breakdown path), the real input x[1], and the oracle's / the truth's answer for either.  The device test fills the buffer
  with the decoy, queues  delay + copy of the real input  on the caller's stream and calls the library: it must answer for x[1] at the
  bar the suite already holds that entry to.  The host test asserts that the two answers are at least 1e3 bars apart, so that a
  stale read cannot pass.
"""
import functools
import time

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

from oracle import krylov_oracle as ko
from tests import phi_cases as pc
from tests._util import relerr

N = 4100                 # sparse cases: > 8 tiles of 512 rows (Float64), > 4 of 1024 (Float32), ragged tail
T_STEP = 0.6
TOL = 1e-12              # tests/test_gpu_parity.py: TOL (device vs oracle, 64-bit types)
TOL32_W = 2e-5           # tests/test_gpu_option_forms.py: Problem.bar("w") of the 32-bit types
TOL_DENSE = {"float64": 1e-11, "complex128": 1e-11, "float32": 1e-4, "complex64": 1e-4}      # the dense files' TOL
TOL_MATFREE = 1e-10      # test_matrix_free_operator_on_the_two_kernel_step_odd_sizes
TOL_GEMV = 1e-13         # test_gemv_block_rectangular


def is_complex(T):
    return np.dtype(T).kind == "c"


def krylov_m(T):
    return 12 if is_complex(T) else 20      # complex windows: <= 15 columns on the single-pass step (pipe.hip)


# ------------------------------------------------------------------------------------------- builders
def banded(n, T, seed=0):
    """five diagonals with varying coefficients (the operator of test_native_32bit_single_pass_step): the single-pass step"""
    rng = np.random.default_rng([n, seed])
    d = [0.3 + 0.1 * rng.random(n - 2), 1.2 + 0.1 * rng.random(n - 1), -1.0 + 0.1 * rng.random(n), 0.8 + 0.1 * rng.random(n - 1),
         -0.1 + 0.1 * rng.random(n - 2)]
    A = sp.diags(d, [-2, -1, 0, 1, 2], format="csr")
    if is_complex(T):
        A = A * (1 + 0.25j)
    A = A.tocsr().astype(T)
    A.sort_indices()
    return A


def random_rows(n, T):
    """five entries per row anywhere: no diagonal form, SELL slots"""
    rng = np.random.default_rng(1)
    rows = np.repeat(np.arange(n), 5)
    cols = rng.integers(0, n, 5 * n)
    v = rng.standard_normal(5 * n) * 0.3
    if is_complex(T):
        v = v * (1 + 0.25j)
    A = (sp.csr_matrix((v, (rows, cols)), shape=(n, n)) - 0.5 * sp.eye(n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.astype(T)


def dense_operator(n, T, seed=0):
    rng = np.random.default_rng([n, seed])
    A = -0.5 * np.eye(n) + (rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if is_complex(T) else 0)) / np.sqrt(n)
    return np.asfortranarray(A.astype(T))


def vector(n, T, seed):
    rng = np.random.default_rng([n, 7, seed])
    return (rng.standard_normal(n) + (1j * rng.standard_normal(n) if is_complex(T) else 0)).astype(T)


def hermitian_part(A):
    return ((A + A.conj().T) * 0.5).tocsr()


def wide(T):
    return np.dtype(np.complex128 if is_complex(T) else np.float64)


def err(a, b, mode="rel"):
    """the three error measures of tests/_util.close, and "blocks": the largest relative error over the leading index"""
    a, b = np.asarray(a), np.asarray(b)
    if mode == "abs":
        return float(np.max(np.abs(a - b)))
    if mode == "mat":
        return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))
    if mode == "blocks":
        return max(relerr(x, y) for x, y in zip(a, b))
    return relerr(a, b)


# ------------------------------------------------------------------------------------------- inputs that arrive late
class LateCase:
    def __init__(self, name, bar, mode, x0, x1, answer, **fixed):
        self.name, self.bar, self.mode, self.x, self._answer = name, bar, mode, (x0, x1), answer
        self.__dict__.update(fixed)
        self._want = {}

    def want(self, which):
        """the answer for the decoy (0) or the real input (1): computed once, read-only"""
        if which not in self._want:
            w = np.asarray(self._answer(self.x[which]))
            w.setflags(write=False)
            self._want[which] = w
        return self._want[which]

    def separation(self):
        return err(self.want(0), self.want(1), self.mode)


def _with_values(A, vals):
    A2 = A.copy()
    A2.data = np.asarray(vals, dtype=A.dtype).copy()
    return A2


def _int_matrix(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float64))


@functools.lru_cache(maxsize=None)
def late_cases():
    m = krylov_m(np.float64)
    A = banded(N, np.float64)
    b = vector(N, np.float64, 0)
    out = []
    kw = dict(m=m, ishermitian=False)
    out.append(LateCase("expv_device_b", TOL, "rel", vector(N, np.float64, 1), vector(N, np.float64, 2),
                        lambda x: ko.expv(T_STEP, A, x, **kw), A=A, m=m))

    def basis(x):
        K = ko.arnoldi(A, x, **kw)
        return np.asarray(K.getV())[:, : K.m + 1]
    out.append(LateCase("arnoldi_device_b", TOL, "abs", vector(N, np.float64, 3), vector(N, np.float64, 4), basis, A=A, m=m))
    for name, seed in (("csr_values", 5), ("update_values", 6)):
        rng = np.random.default_rng([N, 7, seed])
        v0 = A.data * (1 + 0.3 * rng.random(A.nnz))
        v1 = A.data * (1 + 0.3 * rng.random(A.nnz))
        out.append(LateCase(name, TOL, "rel", v0, v1, lambda v: ko.expv(T_STEP, _with_values(A, v), b, **kw), A=A, b=b, m=m))
    nd = 130
    bd = vector(nd, np.float64, 0)
    out.append(LateCase("dense_operator", TOL, "rel", dense_operator(nd, np.float64, 1), dense_operator(nd, np.float64, 2),
                        lambda M: ko.expv(T_STEP, M, bd, **kw), b=bd, m=m))
    ne = 96
    out.append(LateCase("exponential", TOL_DENSE["float64"], "rel", np.asfortranarray(np.random.default_rng(1096).standard_normal((ne, ne))),
                        np.asfortranarray(np.random.default_rng(1097).standard_normal((ne, ne))), lambda M: sl.expm(M.astype(np.complex128))))
    out.append(LateCase("phi", TOL_DENSE["float64"], "blocks", np.array(pc.matrix("float64", ne, 2.0, "randn", seed=11)),
                        np.array(pc.matrix("float64", ne, 2.0, "randn", seed=12)), lambda M: np.stack(pc.truth(M, 2)), k=2))
    Am = _int_matrix((130, 96), 21)
    out.append(LateCase("mul", 0.0, "abs", _int_matrix((96, 130), 22), _int_matrix((96, 130), 23), lambda B: Am @ B, A=Am))
    Ag = np.asfortranarray(np.random.default_rng(24).standard_normal((130, 96)))
    out.append(LateCase("gemv_block", TOL_GEMV, "rel", np.random.default_rng(25).standard_normal(96), np.random.default_rng(26).standard_normal(96),
                        lambda x: Ag @ x, A=Ag))
    return {c.name: c for c in out}


# ------------------------------------------------------------------------------------------- the delay
class Delay:
    """A kernel that keeps a stream busy for a given time: torch.cuda._sleep (device clock ticks), a chain of matrix products where this
    build lacks it.  The ticks per millisecond are measured once, with events."""

    def __init__(self, torch):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.per_ms = None
        if self.sleep is None:
            self._a = torch.ones((1024, 1024), device="cuda")

    def _run(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self._a = (self._a @ self._a) * (1.0 / 1024)

    def calibrate(self):
        torch = self.torch
        units = 2_000_000 if self.sleep is not None else 20
        for _ in range(2):          # (the first launch pays for loading the kernel)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._run(units)
            e1.record()
            e1.synchronize()
        self.per_ms = units / max(e0.elapsed_time(e1), 1e-3)
        return self.per_ms

    def enqueue(self, ms):
        """on torch's current stream"""
        if self.per_ms is None:
            self.calibrate()
        self._run(max(1, int(ms * self.per_ms)))


def timed(fn):
    """(result, wall milliseconds) of fn()"""
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)
