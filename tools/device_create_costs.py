"""Creation of a sparse operator from CSR tensors that live on the device, against what the same tensors cost without the device
entry points: .cpu() of the three arrays, a scipy matrix, the host creator.  Counterpart of op_create_costs.py.

    python tools/device_create_costs.py [--out FILE] [--quick]
    python tools/device_create_costs.py --once                 one device creation of the C2 operator (for rocprofv3 --memory-copy-trace)
    python tools/device_create_costs.py --copies DIR           summary of the *memory_copy_trace.csv files under DIR

Per pattern: 3 warm-ups, then 10 timed creations each way, every one ending in ctx.sync(); median with min / max, and the
ingest_info split of the last device creation.  "miss" rows clear the plan cache before every creation (both ways)."""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests._util import c2_operator, stencil2d

eu = expv_mi_loader.load()


def shuffle(A, seed):
    q = np.random.default_rng(seed).permutation(A.shape[0])
    return A[q][:, q].tocsr()


def sprand_gputests(n, per_row=10, seed=0x0451):
    """test/gpu/gputests.jl:41-43"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=per_row / n, random_state=rng, dtype=np.float64) \
        + 1j * sp.random(n, n, density=per_row / n, random_state=rng, dtype=np.float64)
    return (sp.triu(A, 1) + sp.random(n, n, density=1 / n, random_state=rng) * (1 + 1j)).tocsr()


def to_device(A):
    A = A.tocsr()
    A.sort_indices()
    return torch.sparse_csr_tensor(torch.as_tensor(A.indptr), torch.as_tensor(A.indices), torch.as_tensor(A.data), size=A.shape).cuda()


def from_device(At, ctx):
    return eu.MIOperator(At, ctx)


def round_trip(At, ctx):
    """what the same tensors cost through the host creator"""
    S = sp.csr_matrix((At.values().cpu().numpy(), At.col_indices().cpu().numpy(), At.crow_indices().cpu().numpy()), shape=tuple(At.shape))
    return eu.MIOperator(S, ctx)


def timed(f, At, ctx, clear, warm, reps):
    ts, op = [], None
    for i in range(warm + reps):
        op = None
        if clear:
            eu.plan_cache(clear=True)
        torch.cuda.synchronize()
        ctx.sync()
        t0 = time.perf_counter()
        op = f(At, ctx)
        ctx.sync()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return np.array(ts), op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--copies")
    a = ap.parse_args()
    if a.copies:
        return copies(a.copies)
    ctx = eu.Context()
    N = 20_000 if a.quick else 1_000_000
    if a.once:
        At = to_device(c2_operator(N))
        torch.cuda.synchronize()
        op = from_device(At, ctx)
        ctx.sync()
        print("one device creation of the C2 operator, n = %d, nnz = %d: ingest_info %s" % (N, op.nnz, op.ingest_info))
        print("expected device-to-host: %d bytes of pattern (4 (n + 1 + nnz)) + status / property records of a few hundred bytes" % (4 * (N + 1 + op.nnz)))
        return
    k = int(np.sqrt(N))
    cases = [("C2 5 diagonals n=%d" % N, lambda: c2_operator(N), False),
             ("C2 permuted (RCM), plan-cache miss", lambda: shuffle(c2_operator(N), 7), True),
             ("C2 permuted (RCM), plan-cache hit", lambda: shuffle(c2_operator(N), 7), False),
             ("2-D 5-point grid %dx%d (patch), miss" % (k, k), lambda: stencil2d(k), True),
             ("sprand complex n=1000, 10/row", lambda: sprand_gputests(1000), False),
             ("sprand complex n=%d, 10/row" % N, lambda: sprand_gputests(N), False)]
    lines = ["creation of a sparse operator: (a) from device CSR tensors, (b) the same tensors through .cpu() + scipy + the host creator",
             "ms, median [min .. max] of 10 after 3 warm-ups, each ending in ctx.sync(); device: %s" % torch.cuda.get_device_name(0),
             "", "%-44s %10s %26s %26s %7s  %s" % ("pattern", "nnz", "(a) device tensors", "(b) round trip", "b/a", "verdict")]
    for name, make, clear in cases:
        A = make()
        At = to_device(A)
        eu.plan_cache(clear=True)
        ta, op = timed(from_device, At, ctx, clear, 3, 10)
        info = op.ingest_info
        red = op.reorder_info["reordered"], op.patch_info["patch_form"]
        op = None
        tb, _ = timed(round_trip, At, ctx, clear, 3, 10)
        ma, mb = float(np.median(ta)), float(np.median(tb))
        spread = max(ta.max() - ta.min(), tb.max() - tb.min())
        verdict = "not slower" if ma <= mb + spread else "SLOWER"
        lines.append("%-44s %10d %8.2f [%7.2f ..%8.2f] %8.2f [%7.2f ..%8.2f] %7.2f  %s" % (
            name, A.nnz, ma, ta.min(), ta.max(), mb, tb.min(), tb.max(), mb / ma, verdict))
        lines.append("    last device creation: library %.2f ms, of which device checks + status read-back %.3f ms; to the host: pattern %d B, values %d B; "
                     "plan cached %d, reordered %d, patch form %d" % (1e3 * info["create_s"], 1e3 * info["ingest_s"], info["pattern_bytes_to_host"],
                                                                      info["value_bytes_to_host"], info["plan_cached"], red[0], red[1]))
        print("\n".join(lines[-2:]), flush=True)
        del At
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


def copies(d):
    """the copies of a rocprofv3 --memory-copy-trace run, by direction"""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    by = {}
    for r in rows:
        direction = r.get("Direction") or r.get("Name") or "?"
        size = None
        for key in ("Bytes", "Size", "bytes"):      # (the byte column where the version of the tool has one)
            if r.get(key):
                size = int(r[key])
        by.setdefault(direction, []).append(size)
    print("memory copies traced: %d" % len(rows))
    for direction, sizes in sorted(by.items()):
        known = [s for s in sizes if s is not None]
        print("  %-28s %5d copies%s" % (direction, len(sizes), (", %d bytes in all, largest %s" % (sum(known), sorted(known)[-3:])) if known else ""))


if __name__ == "__main__":
    main()
