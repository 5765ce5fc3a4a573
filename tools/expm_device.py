"""Dense exponential on the device (expv_mi_expm) and its product kernel (expv_mi_gemm): what they cost on the MI355X.

    python tools/expm_device.py [--out FILE] [--quick]

Per element type:
  * milliseconds per expv_mi_expm (device-resident matrix, randn / sqrt(n): 1-norm ~ 0.8 sqrt(n)) at n = 64, 256, 1024, 4096 -- warm-up
    calls, then repetitions, each complete on return (the call synchronises); median with min / max;
  * the host routine (expv_mi_host_expm, single thread, same matrix) where n <= 1024, as the baseline;
  * the product kernel's rate at 1024^3 and 4096^3 for BOTH tiles (uniform [-1, 1) operands; a context created under
    EXPV_MI_DENSE_TILE=1 / 2 forces the small / big tile): repetitions enqueued back to back, one synchronise, FLOP = 2 m n k
    (x 4 for the complex types).
Writes profiles/expm_device.txt by default."""
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


def ctx_with_tile(tile):
    old = os.environ.get("EXPV_MI_DENSE_TILE")
    os.environ["EXPV_MI_DENSE_TILE"] = str(tile)
    try:
        return eu.Context()
    finally:
        if old is None:
            del os.environ["EXPV_MI_DENSE_TILE"]
        else:
            os.environ["EXPV_MI_DENSE_TILE"] = old


def randm(rng, shape, T, uniform=False):
    draw = (lambda: rng.uniform(-1, 1, shape)) if uniform else (lambda: rng.standard_normal(shape))
    a = draw()
    if np.dtype(T).kind == "c":
        a = a + 1j * draw()
    return np.asfortranarray(a.astype(T))


def time_expm(ctx, T, n, warm, reps, out):
    lib = eu.api.L.load()
    rng = np.random.default_rng(n)
    A = randm(rng, (n, n), T) / np.sqrt(n).astype(np.dtype(T).char.lower() if np.dtype(T).kind == "f" else np.float64)
    A = np.asfortranarray(A.astype(T))
    src = eu.DeviceArray.from_host(A, ctx)
    work = eu.DeviceArray((n, n), T, ctx)
    info = (C.c_int64 * 8)()
    ts = []
    for i in range(warm + reps):
        eu.api._check(lib.expv_mi_memcpy_h2d(ctx._h, work.ptr, A.ctypes.data, A.nbytes), ctx._h)
        ctx.sync()
        t0 = time.perf_counter()
        eu.api._check(lib.expv_mi_expm(ctx._h, eu.api._code(np.dtype(T)), n, work.ptr, n, 1, info), ctx._h)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append((t1 - t0) * 1e3)
    host = None
    if n <= 1024:
        hr = []
        for _ in range(3 if n <= 256 else 1):
            t0 = time.perf_counter()
            eu.host_expm(A)
            hr.append((time.perf_counter() - t0) * 1e3)
        host = statistics.median(hr)
    out.append("expm  %-10s n=%-5d order=%-2d s=%-2d swaps=%-4d  %9.3f ms  (min %9.3f max %9.3f, %d reps)   host_expm %s" % (
        np.dtype(T).name, n, info[0], info[1], info[2], statistics.median(ts), min(ts), max(ts), reps,
        ("%10.3f ms" % host) if host is not None else "       n/a"))
    print(out[-1], flush=True)
    del src


def time_gemm(ctxs, T, n, reps, out):
    lib = eu.api.L.load()
    rng = np.random.default_rng(7)
    A, B = randm(rng, (n, n), T, True), randm(rng, (n, n), T, True)
    flop = 2.0 * n ** 3 * (4 if np.dtype(T).kind == "c" else 1)
    for tile, ctx in ctxs.items():
        Ad, Bd = eu.DeviceArray.from_host(A, ctx), eu.DeviceArray.from_host(B, ctx)
        Cd = eu.DeviceArray((n, n), T, ctx)
        code = eu.api._code(np.dtype(T))

        def run(k):
            for _ in range(k):
                eu.api._check(lib.expv_mi_gemm(ctx._h, code, n, n, n, 1.0, 0.0, Ad.ptr, n, Bd.ptr, n, 0.0, 0.0, Cd.ptr, n), ctx._h)
            ctx.sync()
        run(2)
        rounds = []
        for _ in range(3):
            t0 = time.perf_counter()
            run(reps)
            rounds.append((time.perf_counter() - t0) / reps)
        t = statistics.median(rounds)
        out.append("gemm  %-10s %d^3  tile=%-5s  %9.3f ms  %8.2f TFLOP/s  (min %.3f ms, 3 rounds of %d)" % (
            np.dtype(T).name, n, tile, t * 1e3, flop / t / 1e12, min(rounds) * 1e3, reps))
        print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expm_device.txt"))
    ap.add_argument("--quick", action="store_true", help="sizes up to 1024 only")
    args = ap.parse_args()
    out = ["# tools/expm_device.py on the MI355X: expv_mi_expm per call and expv_mi_gemm rate per tile (see the tool's docstring)"]
    ctx = eu.Context()
    ctxs = {"small": ctx_with_tile(1), "big": ctx_with_tile(2)}
    sizes = [64, 256, 1024] + ([] if args.quick else [4096])
    for T in TYPES:
        for n in sizes:
            time_expm(ctx, T, n, 3 if n <= 1024 else 1, 10 if n <= 1024 else 3, out)
    for T in TYPES:
        for n in ([1024] if args.quick else [1024, 4096]):
            time_gemm(ctxs, T, n, 20 if n <= 1024 else 5, out)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
