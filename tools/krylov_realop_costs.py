"""What the Krylov expv(-i tau A, b) costs on a REAL operator with a complex b as a mixed call (keep_real=True: the operator as it
is stored) beside the same call on the operator promoted to the complex type -- the alternative without it.

    python tools/krylov_realop_costs.py [--out FILE] [--quick]

n = 10^6, m = 30, tol 1e-7, Float64 and Float32, complex vectors on the device, on
    the symmetric 5-diagonal operator (lanczos!: a real tridiagonal H under a complex basis), and
    8 random entries per row (arnoldi!, full window).
Two calls, interleaved in one process (a, b, a, b, ...), 2 warm-up rounds and the median [min .. max] of 7 timed ones, each call
complete on return:
    (a) expv(t, op, b, keep_real=True)            the mixed call: two-kernel step, the operator walked in its real type;
    (b) expv(t, op.astype(complex), b)            the promoted copy, built once outside the timing.
Per call: ms, the step form it took, per-kernel times from the context's profiler (a separate, untimed call with the profiler on),
and how far (a) is from (b).  Per operator: the creation time of the promoted copy and the device memory both operators take (the
drop of free device memory around the creation).  Expectation: on the band the promoted copy runs the single-pass step, which the
mixed call has no form of -- it may well be slower there; on general sparse rows both run a two-kernel step and the mixed one reads
half the operator's value bytes.  These are measurements, not targets."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import expv_mi_loader
from tests._util import c2_operator
from tools.expv_taylor_costs import random_sparse

eu = expv_mi_loader.load()
M = 30


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def created(make, ctx):
    ctx.sync()
    f0, t0 = free_bytes(), time.perf_counter()
    op = make()
    ctx.sync()
    return op, 1e3 * (time.perf_counter() - t0), f0 - free_bytes()


def kernel_ms(call, ctx):
    """per-kernel totals of one call from the profiler, in a call of its own: {kernel: (launches, ms)}"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    ctx.sync()
    p = ctx.prof_get()
    ctx.prof_enable(False)
    return {k: (v["launches"], v["total_ms"]) for k, v in p.items()}


def relmax(a, b):
    d = float(b.abs().max())
    return float((a - b).abs().max()) / (d if d > 0 else 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "krylov_realop_costs.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 10^5, 3 timed rounds")
    a = ap.parse_args()
    n, warm, reps = (100_000, 1, 3) if a.quick else (1_000_000, 2, 7)
    ctx = eu.default_context()
    lines = ["# Krylov expv(t, A, b), m = %d, tol 1e-7, t = -0.5i, on a real operator with a complex b: the mixed call (keep_real=True) beside the call on the" % M,
             "# promoted complex operator; n = %d, vectors on the device; ms per call = median [min .. max] of %d interleaved rounds; kernels: launches x us each" % (n, reps)]
    for name, A64 in (("symmetric 5 diagonals (lanczos!)", c2_operator(n, sym=True)), ("random sparse, 8 per row (arnoldi!)", random_sparse(n))):
        for R, Cd in ((np.float64, np.complex128), (np.float32, np.complex64)):
            A = A64.astype(R)
            t = -0.5j
            op, ms_r, bytes_r = created(lambda: eu.MIOperator(A, ctx), ctx)
            opc, ms_c, bytes_c = created(lambda: op.astype(Cd), ctx)
            b = torch.as_tensor(np.random.default_rng(3).standard_normal(n).astype(R) + 1j * np.random.default_rng(4).standard_normal(n).astype(R)).cuda()
            calls = {"mixed": lambda: eu.expv(t, op, b, m=M, tol=1e-7, keep_real=True),
                     "promoted": lambda: eu.expv(t, opc, b, m=M, tol=1e-7)}
            ts = {k: [] for k in calls}
            out, path = {}, {}
            for i in range(warm + reps):
                for k, f in calls.items():      # interleaved: a, b, a, b, ...
                    ctx.sync()
                    t0 = time.perf_counter()
                    out[k] = f()
                    ctx.sync()
                    if i >= warm:
                        ts[k].append(1e3 * (time.perf_counter() - t0))
                    st = eu.expv.last_stats
                    path[k] = "+".join(st["path"]) + (" (real operator)" if st["real_operator"] else "")
            prof = {k: kernel_ms(f, ctx) for k, f in calls.items()}
            med = {k: float(np.median(v)) for k, v in ts.items()}
            lines += ["", "## %s, %s: nnz = %d; real operator %.1f MB (created in %.0f ms), promoted copy %.1f MB more (made in %.0f ms)"
                      % (name, np.dtype(R).name, A.nnz, bytes_r / 1e6, ms_r, bytes_c / 1e6, ms_c),
                      "%-9s %-30s %-36s %s" % ("call", "ms per call", "step form", "kernels")]
            for k in calls:
                v = np.array(ts[k])
                ker = "  ".join("%s %d x %.1f" % (q, l, 1e3 * ms / max(l, 1)) for q, (l, ms) in sorted(prof[k].items()))
                lines.append("%-9s %-30s %-36s %s" % (k, "%8.2f [%7.2f .. %7.2f]" % (np.median(v), v.min(), v.max()), path[k], ker))
            lines.append("mixed / promoted: %.3f in ms per call; mixed against promoted, relative in the max norm: %.2e"
                         % (med["mixed"] / med["promoted"], relmax(out["mixed"], out["promoted"])))
            print("\n".join(lines[-5:]), flush=True)
            del op, opc
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
