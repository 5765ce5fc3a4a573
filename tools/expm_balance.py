"""Balanced against unbalanced dense exponential on the device (expv_mi_expm_balanced / expv_mi_expm): what balancing costs on a
well-scaled matrix and what it saves on a badly scaled one, on the MI355X.

    python tools/expm_balance.py [--out FILE] [--quick]

Per element type and n = 64, 256, 1024, 4096, on two inputs built from the same B (randn scaled to |B|_1 = 2):
  * "well":   A = B;
  * "scaled": A = D B D^-1, D = diag(2^e_i), e_i uniform integers in [-20, 20] (tests/balance_cases.py's `scaled`, without its truth),
the milliseconds of a whole call of either entry (device-resident matrix, warm-up calls, then repetitions, each complete on return;
median), the squarings each one needs, and for the balanced entry the share of the call spent balancing and undoing it (info[7]) and
the sweeps of the scaling loop.
Writes profiles/expm_balance.txt by default."""
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


def inputs(T, n):
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n))
    if np.dtype(T).kind == "c":
        B = B + 1j * rng.standard_normal((n, n))
    B = (B * (2.0 / np.linalg.norm(B, 1))).astype(T)
    D = np.ldexp(1.0, rng.integers(-20, 21, size=n))
    wide = np.complex128 if np.dtype(T).kind == "c" else np.float64
    A = (B.astype(wide) * D[:, None] / D[None, :]).astype(T)
    return {"well": np.asfortranarray(B), "scaled": np.asfortranarray(A)}


def time_entry(ctx, fn, T, A, warm, reps):
    lib = eu.api.L.load()
    n = A.shape[0]
    work = eu.DeviceArray((n, n), T, ctx)
    info = (C.c_int64 * 8)()
    ts, share = [], []
    for i in range(warm + reps):
        eu.api._check(lib.expv_mi_memcpy_h2d(ctx._h, work.ptr, A.ctypes.data, A.nbytes), ctx._h)
        ctx.sync()
        t0 = time.perf_counter()
        eu.api._check(fn(ctx._h, eu.api._code(np.dtype(T)), n, work.ptr, n, 1, info), ctx._h)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append((t1 - t0) * 1e3)
            share.append(info[7] / 1e3)
    return statistics.median(ts), min(ts), statistics.median(share), list(info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expm_balance.txt"))
    ap.add_argument("--quick", action="store_true", help="sizes up to 1024 only")
    args = ap.parse_args()
    lib = eu.api.L.load()
    out = ["# tools/expm_balance.py on the MI355X: expv_mi_expm against expv_mi_expm_balanced, ms per call (see the tool's docstring)",
           "# %-10s %5s %-7s | %-22s | %s" % ("dtype", "n", "input", "expv_mi_expm: ms (s)", "expv_mi_expm_balanced: ms (s), of which balancing ms, sweeps")]
    ctx = eu.Context()
    sizes = [64, 256, 1024] + ([] if args.quick else [4096])
    for T in TYPES:
        for n in sizes:
            warm, reps = (2, 7) if n <= 1024 else (1, 3)
            for name, A in inputs(T, n).items():
                u_ms, u_min, _, uinfo = time_entry(ctx, lib.expv_mi_expm, T, A, warm, reps)
                b_ms, b_min, b_bal, binfo = time_entry(ctx, lib.expv_mi_expm_balanced, T, A, warm, reps)
                out.append("%-12s %5d %-7s | %9.3f (s = %2d)      | %9.3f (s = %2d), balancing %9.3f (%4.1f %%), %2d sweeps" % (
                    np.dtype(T).name, n, name, u_ms, uinfo[1], b_ms, binfo[1], b_bal, 100.0 * b_bal / b_ms, binfo[6]))
                print(out[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
