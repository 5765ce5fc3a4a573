"""Creation of a sparse operator from stored diagonals that live on the device (expv_mi_op_create_dia_loc, MIOperator.from_dia),
against what the same caller had before.  Counterpart of bsr_create_costs.py.

    python tools/dia_create_costs.py [--out FILE] [--quick]

Per case (n = 10^6; 5 diagonals -- the headline operator -- and 25; Float64 and ComplexF64; column alignment, ld = n):
  (a) from_dia(device tensor) against MIOperator(torch.sparse_csr tensor) of the equivalent CSR arrays ALREADY on the device
      (expv_mi_op_create_csr_loc, which this creator leaves as it was): the whole creation and the ingest stage
      (ingest_info: create_s, ingest_s).  3 warm-ups, 10 timed creations each, every one ending in ctx.sync(); median [min .. max].
  (b) scipy's dia_matrix.tocsr() on the host plus the host creator MIOperator(csr): 1 warm-up, 3 timed.
  (c) a value refresh through update_values, by device events on a context that works on a torch stream: diagonal-born against
      CSR-born, 3 warm-ups, 20 timed each.
  (d) the value transposition (op_dia.hip: k_dia_vals) alone: the two refreshes of (c) differ by that one launch, so its time is the
      difference of their medians ("inside the spread" when it does not exceed the larger min-max spread); its rate
      2 * value bytes * nnz / time against a device-to-device hipMemcpyAsync of value bytes * nnz (the same bytes read and written)
      on the same stream in the same run, by device events, 3 warm-ups, 20 timed."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import expv_mi_loader

eu = expv_mi_loader.load()


def timed(make, ctx, warm, reps):
    ts, stage, op = [], [], None
    for i in range(warm + reps):
        op = None
        torch.cuda.synchronize()
        ctx.sync()
        t0 = time.perf_counter()
        op = make(ctx)
        ctx.sync()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
            stage.append(1e3 * op.ingest_info["ingest_s"])
    return np.array(ts), np.array(stage), op


def by_events(f, S, warm, reps):
    out = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(S)
        f()
        e1.record(S)
        e1.synchronize()
        if i >= warm:
            out.append(e0.elapsed_time(e1))
    return np.array(out)


def fmt(t):
    return "%8.3f [%8.3f ..%8.3f]" % (float(np.median(t)), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    a = ap.parse_args()
    n = 20_000 if a.quick else 1_000_000
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    ctx = eu.Context()
    S = torch.cuda.Stream()
    ctx_s = eu.Context(stream=S)
    lines = ["creation of a sparse operator from stored diagonals on the device: (a) MIOperator.from_dia(device tensor) vs MIOperator(device CSR tensor),",
             "(b) dia_matrix.tocsr() + host creator, (c) update_values, (d) the value transposition against a device-to-device copy",
             "ms, median [min .. max]; device: %s; torch %s; n = %d" % (torch.cuda.get_device_name(0), torch.__version__, n), ""]
    for nd in (5, 25):
        for T in (np.float64, np.complex128):
            offs = [k - nd // 2 for k in range(nd)] if nd == 5 else [s * k for k in (1, 2, 3, 4, 100, 200) for s in (-1, 1)] + \
                [0] + [s * k for k in (1000, 1001, 1002, 2000, 2001, 2002) for s in (-1, 1)]
            assert len(offs) == nd == len(set(offs))
            rng = np.random.default_rng(nd)
            data = rng.standard_normal((nd, n)).astype(T)
            if np.dtype(T).kind == "c":
                data = data + 1j * rng.standard_normal((nd, n))
            D = sp.dia_matrix((data, offs), shape=(n, n))
            t0 = time.perf_counter()
            M = D.tocsr()
            t_tocsr = 1e3 * (time.perf_counter() - t0)
            M.sort_indices()
            dt = torch.as_tensor(data).cuda()
            Mt = torch.sparse_csr_tensor(torch.as_tensor(M.indptr).cuda(), torch.as_tensor(M.indices).cuda(), torch.as_tensor(M.data).cuda(), size=M.shape)
            torch.cuda.synchronize()
            eu.plan_cache(clear=True)
            ta, sa, op = timed(lambda c: eu.MIOperator.from_dia(dt, offs, n, "col", ctx=c), ctx, 3, 10)
            info, nnz, v = op.ingest_info, op.nnz, op.dtype.itemsize
            assert nnz == M.nnz
            op = None
            tc, sc, opc = timed(lambda c: eu.MIOperator(Mt, c), ctx, 3, 10)
            opc = None
            th, _, oph = timed(lambda c: eu.MIOperator(sp.dia_matrix((data, offs), shape=(n, n)).tocsr(), c), ctx, 1, 3)
            oph = None
            spread = max(np.ptp(ta), np.ptp(tc))
            slower = np.median(ta) > np.median(tc) + spread or ta.min() > tc.max()
            lines.append("%d diagonals %s: nnz %d" % (nd, np.dtype(T).name, nnz))
            lines.append("    (a) from_dia(device)      %s   ingest stage (table, expansion, transposition; host clock) %s; pattern to the host %d B; plan cached %d" % (
                fmt(ta), fmt(sa), info["pattern_bytes_to_host"], info["plan_cached"]))
            lines.append("        MIOperator(device CSR) %s   ingest stage (checks, status read-back) %s" % (fmt(tc), fmt(sc)))
            lines.append("        csr/dia %.2f  %s (spread of the run %.3f ms)" % (np.median(tc) / np.median(ta), "SLOWER" if slower else "not slower", spread))
            lines.append("    (b) dia_matrix.tocsr() + host creator %s   (tocsr alone %.1f ms)" % (fmt(th), t_tocsr))
            opa, opb = eu.MIOperator.from_dia(dt, offs, n, "col", ctx=ctx_s), eu.MIOperator(Mt, ctx_s)
            d2, v2 = dt * 1.5, torch.as_tensor(M.data).cuda() * 1.5
            dst = torch.empty_like(v2)
            torch.cuda.synchronize()
            ra = by_events(lambda: opa.update_values(d2), S, 3, 20)
            rb = by_events(lambda: opb.update_values(v2), S, 3, 20)
            nbytes = v * nnz
            rm = by_events(lambda: hip.hipMemcpyAsync(dst.data_ptr(), v2.data_ptr(), nbytes, 3, S.cuda_stream), S, 3, 20)
            d = float(np.median(ra)) - float(np.median(rb))
            lines.append("    (c) update_values, device events: diagonal-born %s, CSR-born %s" % (fmt(ra), fmt(rb)))
            known = d > max(np.ptp(ra), np.ptp(rb))
            lines.append("    (d) k_dia_vals = difference of the medians %.3f ms for 2 * %d B * nnz = %.1f MB -> %s; hipMemcpyAsync D2D of %.1f MB %s -> %.0f GB/s%s" % (
                d, v, 2e-6 * nbytes, "%.0f GB/s" % (2e-6 * nbytes / d) if known else "inside the spread", 1e-6 * nbytes, fmt(rm),
                2e-6 * nbytes / float(np.median(rm)),
                ("; kernel / copy = %.2f%s" % (float(np.median(rm)) / d, "  BELOW HALF THE COPY'S RATE" if 2 * float(np.median(rm)) < d else "")) if known else ""))
            print("\n".join(lines[-7:]), flush=True)
            del opa, opb, dt, Mt, d2, v2, dst
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
