"""Creation of a linear combination of operators that exist (expv_mi_op_create_lincomb, MIOperator.lincomb) and the change of a
coefficient (expv_mi_op_lincomb_refresh, MIOperator.recombine), against the floor and against what the same caller had before.
Counterpart of adjoint_create_costs.py.

    python tools/lincomb_costs.py [--out FILE] [--quick]

Cases (n = 10^6, Float64 and ComplexF64): two 5-diagonal terms with different offsets (the union has 8 diagonals), and two terms
of 8 random entries per row each.  Per case, C = A + f B:
  (a) MIOperator.lincomb([A, B], [1, f]): the first creation after the plan cache was cleared, then 3 warm-ups and 10 timed
      creations on the cached pattern, every one ending in ctx.sync(); median [min .. max]; the ingest stage (keys, sort, heads,
      compression, gather-scale-sum; host clock) beside it.
  (b) C.recombine([1, f']) by device events on a context that works on a torch stream: 3 warm-ups, 20 timed.
  (c) the floor: C.update_values(nnz values on the device, in C's order), the same way.  (b) and (c) differ by the
      gather-scale-sum launch.
  (d) what a caller does today: the sum made by torch on the device (sparse_coo addition, coalesce, conversion to CSR), the old
      operator dropped and MIOperator(CSR tensor) created; 3 warm-ups, 10 timed, host clock; torch's share beside it."""
import argparse
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


def csr_tensor(M):
    return torch.sparse_csr_tensor(torch.as_tensor(M.indptr).cuda(), torch.as_tensor(M.indices).cuda(), torch.as_tensor(M.data).cuda(), size=M.shape)


def coo_tensor(M):
    C = M.tocoo()
    idx = torch.as_tensor(np.vstack([C.row, C.col]).astype(np.int64)).cuda()
    return torch.sparse_coo_tensor(idx, torch.as_tensor(C.data).cuda(), size=M.shape).coalesce()


def cases(n, T):
    rng = np.random.default_rng(5)
    pairs = (("two 5-diagonal terms", sp.diags([0.3, 1.2, -2.0, 0.8, -0.1], [-2, -1, 0, 1, 2], shape=(n, n), format="csr"),
              sp.diags([0.2, -0.7, 0.5, 0.4, -0.3], [-5, -1, 0, 1, 5], shape=(n, n), format="csr")),
             ("two terms of 8 random entries per row", sp.random(n, n, density=8.0 / n, random_state=rng, format="csr"),
              sp.random(n, n, density=8.0 / n, random_state=rng, format="csr")))
    for name, A, B in pairs:
        out = []
        for M in (A, B):
            M = M.astype(T)
            if np.dtype(T).kind == "c":
                M.data = M.data * (1.0 + 0.25j * np.cos(np.arange(M.nnz)))
            M.sort_indices()
            out.append(M)
        yield name, out[0], out[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    a = ap.parse_args()
    n = 20_000 if a.quick else 1_000_000
    ctx = eu.Context()
    S = torch.cuda.Stream()
    ctx_s = eu.Context(stream=S)
    lines = ["C = A + f B of two existing operators on the device: (a) MIOperator.lincomb, first and on a cached pattern; (b) C.recombine(new f)",
             "and (c) C.update_values(values), device events; (d) today's way: torch's sparse sum on the device + MIOperator(CSR tensor)",
             "ms, median [min .. max]; device: %s; torch %s; n = %d" % (torch.cuda.get_device_name(0), torch.__version__, n), ""]
    for T in (np.float64, np.complex128):
        for name, A, B in cases(n, T):
            At, Bt = csr_tensor(A), csr_tensor(B)
            torch.cuda.synchronize()
            pa, pb = eu.MIOperator(At, ctx), eu.MIOperator(Bt, ctx)
            eu.plan_cache(clear=True)
            t1, s1, op = timed(lambda c: eu.MIOperator.lincomb([pa, pb], [1.0, 0.5]), ctx, 0, 1)
            first_cached = op.ingest_info["plan_cached"]
            ta, sa, op = timed(lambda c: eu.MIOperator.lincomb([pa, pb], [1.0, 0.5]), ctx, 3, 10)
            info = op.ingest_info
            nnz = op.nnz
            op = None
            lines.append("%s %s: nnz %d + %d -> %d" % (name, np.dtype(T).name, A.nnz, B.nnz, nnz))
            lines.append("    (a) lincomb first  %8.3f   ingest stage %8.3f; plan cached %d" % (t1[0], s1[0], first_cached))
            lines.append("        lincomb cached %s   ingest stage (keys, sort, heads, compression, gather-scale-sum; host clock) %s; pattern to the host %d B; plan cached %d" % (
                fmt(ta), fmt(sa), info["pattern_bytes_to_host"], info["plan_cached"]))
            qa, qb = eu.MIOperator(At, ctx_s), eu.MIOperator(Bt, ctx_s)
            comb = eu.MIOperator.lincomb([qa, qb], [1.0, 0.5])
            vals = torch.zeros(nnz, dtype=At.values().dtype, device="cuda") + 1
            torch.cuda.synchronize()
            f = [0.5]

            def again():
                f[0] += 0.125
                comb.recombine([1.0, f[0]])

            rb = by_events(again, S, 3, 20)
            rc = by_events(lambda: comb.update_values(vals), S, 3, 20)
            lines.append("    (b) device events: C.recombine([1, f]) %s" % fmt(rb))
            lines.append("    (c) device events: C.update_values(values) %s   (b) - (c), medians: %.3f" % (fmt(rc), float(np.median(rb) - np.median(rc))))
            try:
                Ac, Bc = coo_tensor(A), coo_tensor(B)
                torch.cuda.synchronize()
                share = []

                def today(c):
                    t0 = time.perf_counter()
                    Ct = (Ac + 0.5 * Bc).coalesce().to_sparse_csr()
                    torch.cuda.synchronize()
                    share.append(1e3 * (time.perf_counter() - t0))
                    return eu.MIOperator(Ct, c)

                td, _, opd = timed(today, ctx, 3, 10)
                assert opd.nnz == nnz, (opd.nnz, nnz)
                opd = None
                lines.append("    (d) torch sum + MIOperator(CSR tensor) %s   of which torch's sum %s" % (fmt(td), fmt(np.array(share[3:]))))
            except Exception as e:      # (a torch build without the sparse kernels: say so, keep the rest of the record)
                lines.append("    (d) not measured: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:160]))
            print("\n".join(lines[-6:]), flush=True)
            del pa, pb, qa, qb, comb, At, Bt, vals
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
