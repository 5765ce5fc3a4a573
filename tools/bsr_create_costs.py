"""Creation of a sparse operator from a torch.sparse_bsr tensor that lives on the device (expv_mi_op_create_bsr_loc), against the
route the same tensor needed before: conversion to CSR in torch, then the CSR creator.  Counterpart of coo_create_costs.py.

    python tools/bsr_create_costs.py [--out FILE] [--quick]

Per pattern: 3 warm-ups, then 10 timed creations each way, every one ending in ctx.sync(); median with min / max.  (a) counts as
slower when its median exceeds (b)'s by more than the larger min-max spread of the two, or when its fastest creation is slower than
(b)'s slowest.  Route (b) tries the conversions torch may offer for a device BSR tensor, in the order of CONVERSIONS below, and says which one it used; when torch
offers none on the device the tensor goes through the host (scipy's tocsr) -- the round trip the issue speaks of.

The value-permutation pass of update_values (op_bsr.hip: k_bsr_vals) is reported on its own: on a context that works on a torch
stream, device events around update_values(device values) of the block-born operator and of the CSR-born operator of the same
scalar arrays -- the two differ by that one launch -- 20 times each; the difference of the medians against the model
2 * (bytes of a value) * nnz, or "inside the spread" when it does not exceed the larger min-max spread of the two."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests._util import stencil2d
from tests.bsr_cases import from_block_pattern, scalar_matrix

eu = expv_mi_loader.load()

CONVERSIONS = [("A.to_sparse_csr()", lambda A: A.to_sparse_csr()),
               ("A.to_sparse_coo().to_sparse_csr()", lambda A: A.to_sparse_coo().to_sparse_csr())]


def bsr_tensor(ptr, idx, vals):
    n = (len(ptr) - 1) * vals.shape[1]
    return torch.sparse_bsr_tensor(torch.as_tensor(ptr).cuda(), torch.as_tensor(idx).cuda(), torch.as_tensor(vals).cuda(), size=(n, n))


def through_host(At):
    ptr, idx, vals = At.crow_indices().cpu().numpy(), At.col_indices().cpu().numpy(), At.values().cpu().numpy()
    return sp.bsr_matrix((vals, idx, ptr), shape=tuple(At.shape)).tocsr()


def pick_conversion(At):
    """the first conversion torch performs for this tensor on the device, or the host round trip"""
    for name, f in CONVERSIONS:
        try:
            C = f(At)
            if C.layout == torch.sparse_csr and C.is_cuda:
                return name, f
        except (RuntimeError, NotImplementedError) as e:
            print("    torch refuses %s: %s" % (name, str(e).splitlines()[0][:120]), flush=True)
    return "A -> host, scipy bsr_matrix.tocsr(), host creator (torch converts no device BSR tensor to CSR)", through_host


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


def refresh_ms(op, v, S, reps=20):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(S)
        op.update_values(v)
        e1.record(S)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.array(out)


def fmt(t):
    return "%8.3f [%8.3f ..%8.3f]" % (float(np.median(t)), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    a = ap.parse_args()
    ctx = eu.Context()
    nb3, k = (7_000, 64) if a.quick else (333_334, 707)
    tri = sp.diags([np.ones(nb3 - 1), np.ones(nb3), np.ones(nb3 - 1)], [-1, 0, 1])
    cases = [("block-tridiagonal bd=3 fp64, n=%d" % (3 * nb3), lambda: from_block_pattern(tri, 3, np.float64, 1)),
             ("two species on a %d x %d grid, bd=2 fp64, n=%d" % (k, k, 2 * k * k), lambda: from_block_pattern(stencil2d(k), 2, np.float64, 2)),
             ("two species on a %d x %d grid, bd=2 fp32, n=%d" % (k, k, 2 * k * k), lambda: from_block_pattern(stencil2d(k), 2, np.float32, 2))]
    lines = ["creation of a sparse operator from a device torch.sparse_bsr tensor: (a) MIOperator.from_bsr(tensor), (b) conversion to CSR + MIOperator",
             "ms, median [min .. max] of 10 after 3 warm-ups, each ending in ctx.sync(); device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    S = torch.cuda.Stream()
    ctx_s = eu.Context(stream=S)
    for name, make in cases:
        ptr, idx, vals = make()
        At = bsr_tensor(ptr, idx, vals)
        torch.cuda.synchronize()
        how, conv = pick_conversion(At)
        eu.plan_cache(clear=True)
        ta, sa, op = timed(lambda A, c: eu.MIOperator.from_bsr(A, ctx=c), At, ctx, 3, 10)
        info, nnz, v = op.ingest_info, op.nnz, op.dtype.itemsize
        op = None
        tb, _, opb = timed(lambda A, c: eu.MIOperator(conv(A), c), At, ctx, 3, 10)
        nnz_b = opb.nnz
        opb = None
        ma, mb = float(np.median(ta)), float(np.median(tb))
        spread = max(ta.max() - ta.min(), tb.max() - tb.min())
        lines.append("%s: %d blocks, nnz %d" % (name, len(idx), nnz))
        lines.append("    (a) from_bsr            %s   device stage (staging buffers, checks, expansion, permutation; host clock) %s ms; pattern to the host %d B; plan cached %d" % (
            fmt(ta), fmt(sa), info["pattern_bytes_to_host"], info["plan_cached"]))
        lines.append("    (b) %s  %s   nnz %d" % (how, fmt(tb), nnz_b))
        slower = ma > mb + spread or ta.min() > tb.max()      # beyond the spread, or every (a) slower than every (b)
        lines.append("    b/a %.2f  %s (spread of the run %.3f ms)" % (mb / ma, "SLOWER" if slower else "not slower", spread))
        # the permutation pass of a value refresh, by subtraction of two event-timed refreshes
        opa = eu.MIOperator.from_bsr(At, ctx=ctx_s)
        M = scalar_matrix(ptr, idx, vals, vals.shape[1])
        opc = eu.MIOperator(torch.sparse_csr_tensor(torch.as_tensor(M.indptr).cuda(), torch.as_tensor(M.indices).cuda(), torch.as_tensor(M.data).cuda(),
                                                    size=M.shape), ctx_s)
        va, vc = At.values().contiguous() * 1.5, torch.as_tensor(M.data).cuda() * 1.5
        torch.cuda.synchronize()
        refresh_ms(opa, va, S, 3), refresh_ms(opc, vc, S, 3)
        ra, rc = refresh_ms(opa, va, S), refresh_ms(opc, vc, S)
        d = float(np.median(ra)) - float(np.median(rc))
        model = 2.0 * v * nnz
        lines.append("    update_values, device events: block-born %s, CSR-born %s ms; permutation pass = difference of the medians %.3f ms; "
                     "model 2 * %d B * nnz = %.1f MB -> %s" % (fmt(ra), fmt(rc), d, v, 1e-6 * model,
                                                              "%.0f GB/s" % (1e-6 * model / d) if d > max(np.ptp(ra), np.ptp(rc)) else "inside the spread"))
        print("\n".join(lines[-5:]), flush=True)
        del At, opa, opc
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
