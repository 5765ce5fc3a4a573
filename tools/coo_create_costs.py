"""Creation of a sparse operator from a torch.sparse_coo tensor that lives on the device (expv_mi_op_create_coo_loc), against the
route the same tensor needed before: A.coalesce().to_sparse_csr() in torch, then the CSR creator.  Counterpart of
device_create_costs.py.

    python tools/coo_create_costs.py [--out FILE] [--quick]

Per pattern: 3 warm-ups, then 10 timed creations each way, every one ending in ctx.sync(); median with min / max.  For route (a)
also the time inside the triplet stage (check + key, sort, heads + compress, segment sums and the two status read-backs between
them), taken by the library from HIP events around it (ingest_info["ingest_s"]), and the bytes that stage moves by the model
    entries * (24 key pass + 24 * sort passes + 8 heads) + stored * (8 colind / seg) + entries * (4 + v) + stored * v for the sums
(the histogram launch of every sort pass reads the keys once more: 8 B * entries * passes, not in the model)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests._util import c2_operator
from tests.coo_cases import split_triplets

eu = expv_mi_loader.load()


def sprand_gputests(n, per_row=10, seed=0x0451):
    """test/gpu/gputests.jl:41-43"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=per_row / n, random_state=rng, dtype=np.float64) \
        + 1j * sp.random(n, n, density=per_row / n, random_state=rng, dtype=np.float64)
    return (sp.triu(A, 1) + sp.random(n, n, density=1 / n, random_state=rng) * (1 + 1j)).tocsr()


def shuffled(A, share=0.10):
    row, col, vals = split_triplets(A, share, "exact", 5)
    return torch.sparse_coo_tensor(torch.as_tensor(np.vstack([row, col])), torch.as_tensor(vals), size=A.shape).cuda()


def coalesced(A):
    C = A.tocsr().tocoo()
    return torch.sparse_coo_tensor(torch.as_tensor(np.vstack([C.row, C.col]).astype(np.int64)), torch.as_tensor(C.data), size=A.shape).cuda().coalesce()


def from_coo(At, ctx):
    return eu.MIOperator.from_coo(At, ctx=ctx)


def through_torch_csr(At, ctx):
    """what the parent commit offered: coalesce, sort and compress in torch, then the device CSR creator"""
    return eu.MIOperator(At.coalesce().to_sparse_csr(), ctx)


def timed(f, At, ctx, warm, reps):
    ts, stage, op = [], [], None
    for i in range(warm + reps):
        op = None
        torch.cuda.synchronize()
        ctx.sync()
        t0 = time.perf_counter()
        op = f(At, ctx)
        ctx.sync()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
            stage.append(1e3 * op.ingest_info["ingest_s"])
    return np.array(ts), np.array(stage), op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    a = ap.parse_args()
    ctx = eu.Context()
    N = 20_000 if a.quick else 1_000_000
    cases = [("C2 n=%d shuffled, 10%% repeats" % N, lambda: shuffled(c2_operator(N))),
             ("C2 n=%d coalesced (skip path)" % N, lambda: coalesced(c2_operator(N))),
             ("sprand complex n=%d, 10/row, shuffled, 10%% repeats" % N, lambda: shuffled(sprand_gputests(N))),
             ("sprand complex n=1000, 10/row, shuffled, 10% repeats", lambda: shuffled(sprand_gputests(1000)))]
    lines = ["creation of a sparse operator from a device torch.sparse_coo tensor: (a) MIOperator.from_coo(tensor), (b) tensor.coalesce().to_sparse_csr() + MIOperator",
             "ms, median [min .. max] of 10 after 3 warm-ups, each ending in ctx.sync(); device: %s" % torch.cuda.get_device_name(0),
             "", "%-52s %10s %10s %26s %26s %7s  %s" % ("pattern", "entries", "stored", "(a) triplets", "(b) torch coalesce + CSR", "b/a", "verdict")]
    for name, make in cases:
        At = make()
        torch.cuda.synchronize()
        eu.plan_cache(clear=True)
        ta, sa, op = timed(from_coo, At, ctx, 3, 10)
        info, stored, v = op.ingest_info, op.nnz, op.dtype.itemsize
        op = None
        tb, _, _ = timed(through_torch_csr, At, ctx, 3, 10)
        ma, mb = float(np.median(ta)), float(np.median(tb))
        spread = max(ta.max() - ta.min(), tb.max() - tb.min())
        verdict = "not slower" if ma <= mb + spread else "SLOWER"
        ent, passes = info["coo_entries"], info["sort_passes"]
        summed = stored < ent or passes > 0
        model = ent * (24 + 24 * passes + 8) + stored * 8 + (ent * (4 + v) + stored * v if summed else 0)
        ms = float(np.median(sa))
        lines.append("%-52s %10d %10d %8.2f [%7.2f ..%8.2f] %8.2f [%7.2f ..%8.2f] %7.2f  %s" % (
            name, ent, stored, ma, ta.min(), ta.max(), mb, tb.min(), tb.max(), mb / ma, verdict))
        lines.append("    triplet stage (HIP events): %.3f ms median [%.3f .. %.3f] = %.0f %% of (a); %d sort passes; model %.1f MB -> %.0f GB/s; "
                     "rest of (a): pattern to the host (%d B), planners, fill of the stored forms; plan cached %d" % (
                         ms, sa.min(), sa.max(), 100 * ms / ma, passes, 1e-6 * model, 1e-6 * model / max(ms, 1e-9), info["pattern_bytes_to_host"],
                         info["plan_cached"]))
        print("\n".join(lines[-2:]), flush=True)
        del At
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
