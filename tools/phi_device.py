"""Dense phi functions on the device (expv_mi_phi): what a call costs on the MI355X, against the block-augmented exponential.

    python tools/phi_device.py [--out FILE] [--quick]

Per element type, n = 64, 256, 1024, 4096 and k = 1, 4, on a device-resident randn matrix scaled to the 1-norm 5 (s = 3):
  * milliseconds per expv_mi_phi -- warm-up calls, then repetitions, each complete on return (the call synchronises); median with
    min / max;
  * next to it the only other device route to the same matrices: expv_mi_expm of the (k + 1) n block-augmented matrix
    [[A, I, 0, ..], [0, 0, I, ..], ..], whose first block row holds phi_0 .. phi_k (same kernels as before expv_mi_phi existed).
    Run for (k + 1) n <= 5120: above that one augmented exponential takes tens of seconds and six workspace matrices of
    (k + 1)^2 n^2 entries;
  * the recovery pass alone (kernel phi_recover, timed by the context's profiler under "lincomb"): microseconds per launch and the
    rate of its (3 k + 2) n^2 entries of traffic (k old blocks and k + 1 products read, k + 1 blocks written) against HBM_PEAK.
Writes profiles/phi_device.txt by default."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import expv_mi_loader

eu = expv_mi_loader.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [np.float32, np.float64, np.complex64, np.complex128]
HBM_PEAK = 8.0e12          # bytes / s: bench.py's HBM_PEAK_GBS
NORM = 5.0
AUGMENTED_MAX = 5120


def matrix(T, n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n))
    if np.dtype(T).kind == "c":
        a = a + 1j * rng.standard_normal((n, n))
    return np.asfortranarray((a * (NORM / np.linalg.norm(a, 1))).astype(T))


def augmented(A, k):
    n = A.shape[0]
    W = np.zeros(((k + 1) * n, (k + 1) * n), dtype=A.dtype, order="F")
    W[:n, :n] = A
    for j in range(k):
        W[j * n:(j + 1) * n, (j + 1) * n:(j + 2) * n] = np.eye(n, dtype=A.dtype)
    return W


def timed(fn, warm, reps):
    ts = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def measure(ctx, T, n, k, out):
    lib, code = eu.api.L.load(), eu.api._code(np.dtype(T))
    A = matrix(T, n)
    Ad = eu.DeviceArray.from_host(A, ctx)
    slab = eu.DeviceArray((n, (k + 1) * n), T, ctx)
    ptrs = (C.c_void_p * (k + 1))(*[slab.ptr + j * n * n * A.itemsize for j in range(k + 1)])
    info = (C.c_int64 * 8)()
    warm, reps = (3, 10) if n <= 1024 else (1, 3)

    def call():
        eu.api._check(lib.expv_mi_phi(ctx._h, code, n, k, Ad.ptr, n, ptrs, n, 1, info), ctx._h)
    ts = timed(call, warm, reps)
    # the recovery pass alone
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(reps):
        call()
    rec = ctx.prof_get().get("lincomb", {"launches": 0, "total_ms": 0.0})
    launches, ms = rec["launches"], rec["total_ms"]
    ctx.prof_enable(False)
    ctx.prof_reset()
    rec_us = ms * 1e3 / max(launches, 1)
    rate = (3 * k + 2) * n * n * A.itemsize / (rec_us * 1e-6) if rec_us > 0 else 0.0
    # the block-augmented exponential
    aug = "       n/a"
    ratio = ""
    N = (k + 1) * n
    if N <= AUGMENTED_MAX:
        W = augmented(A, k)
        Wd = eu.DeviceArray((N, N), T, ctx)

        def call_aug():
            eu.api._check(lib.expv_mi_memcpy_h2d(ctx._h, Wd.ptr, W.ctypes.data, W.nbytes), ctx._h)
            ctx.sync()
            t0 = time.perf_counter()
            eu.api._check(lib.expv_mi_expm(ctx._h, code, N, Wd.ptr, N, 1, None), ctx._h)
            return (time.perf_counter() - t0) * 1e3
        wa, ra = (2, 5) if N <= 1280 else (1, 2)
        ta = [call_aug() for _ in range(wa + ra)][wa:]
        aug = "%10.3f ms" % statistics.median(ta)
        ratio = "  x%.1f" % (statistics.median(ta) / statistics.median(ts))
        del Wd
    out.append("phi   %-10s n=%-5d k=%d M=%-2d s=%d products=%-2d %9.3f ms  (min %9.3f max %9.3f, %d reps)   augmented expm %s%s   "
               "phi_recover %8.1f us  %6.2f TB/s (%4.1f %% of HBM)" % (
                   np.dtype(T).name, n, k, info[0], info[1], info[2], statistics.median(ts), min(ts), max(ts), reps, aug, ratio,
                   rec_us, rate / 1e12, 100.0 * rate / HBM_PEAK))
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phi_device.txt"))
    ap.add_argument("--quick", action="store_true", help="sizes up to 1024 only")
    args = ap.parse_args()
    out = ["# tools/phi_device.py on the MI355X: expv_mi_phi per call, the block-augmented expv_mi_expm, the recovery pass (see the tool's docstring)"]
    ctx = eu.Context()
    for T in TYPES:
        for n in [64, 256, 1024] + ([] if args.quick else [4096]):
            for k in (1, 4):
                measure(ctx, T, n, k, out)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
