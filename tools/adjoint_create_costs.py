"""Creation of the adjoint of an operator that exists (expv_mi_op_create_adjoint, MIOperator.adjoint) and its refresh
(expv_mi_op_adjoint_refresh, MIOperator.refresh), against what the same caller had before.  Counterpart of dia_create_costs.py.

    python tools/adjoint_create_costs.py [--out FILE] [--quick]

Sparse cases (n = 10^6, Float64 and ComplexF64): the 5-diagonal headline operator, the same band under a random symmetric
permutation (a reordered parent, and an adjoint that is reordered again), 8 random entries per row.  Dense: n = 8192.  Per case
  (a) parent.adjoint(): the first creation after the plan cache was cleared, then 3 warm-ups and 10 timed creations on the cached
      pattern, every one ending in ctx.sync(); median [min .. max]; the ingest stage (keys, sort, pattern, gather; host clock) beside it.
  (b) the same operator through MIOperator(torch.sparse_csr tensor) of the transpose's CSR arrays ALREADY on the device
      (expv_mi_op_create_csr_loc; the transposition itself, done on the host by scipy here, is not in the time): 3 + 10.
      Dense: MIOperator of the packed transposed tensor, and torch's own conj-transpose copy beside it.
  (c) adj.refresh(parent) against adj.update_values(values in the adjoint's order), by device events on a context that works on a
      torch stream: 3 warm-ups, 20 timed each.  The two differ by the gather launch."""
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


def sparse_cases(n, T):
    rng = np.random.default_rng(5)
    band = sp.diags([0.3, 1.2, -2.0, 0.8, -0.1], [-2, -1, 0, 1, 2], shape=(n, n), format="csr")
    q = rng.permutation(n)
    rnd = sp.random(n, n, density=8.0 / n, random_state=rng, format="csr")
    for name, M in (("5 diagonals", band), ("shuffled band", band[q][:, q].tocsr()), ("8 random entries per row", rnd)):
        M = M.astype(T)
        if np.dtype(T).kind == "c":
            M.data = M.data * (1.0 + 0.25j * np.cos(np.arange(M.nnz)))
        M.sort_indices()
        yield name, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    a = ap.parse_args()
    n, nd = (20_000, 512) if a.quick else (1_000_000, 8192)
    ctx = eu.Context()
    S = torch.cuda.Stream()
    ctx_s = eu.Context(stream=S)
    lines = ["creation of the adjoint of an existing operator on the device: (a) parent.adjoint(), first and on a cached pattern, vs",
             "(b) MIOperator(device CSR tensor of the transposed arrays), (c) adj.refresh(parent) vs adj.update_values(values), device events",
             "ms, median [min .. max]; device: %s; torch %s; n = %d (dense: %d)" % (torch.cuda.get_device_name(0), torch.__version__, n, nd), ""]
    for T in (np.float64, np.complex128):
        for name, M in sparse_cases(n, T):
            Mt = M.conj().T.tocsr()
            Mt.sort_indices()
            At, AHt = csr_tensor(M), csr_tensor(Mt)
            torch.cuda.synchronize()
            parent = eu.MIOperator(At, ctx)
            eu.plan_cache(clear=True)
            t1, s1, op = timed(lambda c: parent.adjoint(), ctx, 0, 1)
            first_cached = op.ingest_info["plan_cached"]
            ta, sa, op = timed(lambda c: parent.adjoint(), ctx, 3, 10)
            info = op.ingest_info
            assert op.nnz == M.nnz
            op = None
            eu.plan_cache(clear=True)
            tc1, _, opc = timed(lambda c: eu.MIOperator(AHt, c), ctx, 0, 1)
            tc, sc, opc = timed(lambda c: eu.MIOperator(AHt, c), ctx, 3, 10)
            opc = None
            lines.append("%s %s: nnz %d, parent reordered %d" % (name, np.dtype(T).name, M.nnz, parent.reorder_info["reordered"]))
            lines.append("    (a) parent.adjoint() first  %8.3f   ingest stage %8.3f; plan cached %d" % (t1[0], s1[0], first_cached))
            lines.append("        parent.adjoint() cached %s   ingest stage (keys, sort, pattern, gather; host clock) %s; pattern to the host %d B; plan cached %d" % (
                fmt(ta), fmt(sa), info["pattern_bytes_to_host"], info["plan_cached"]))
            lines.append("    (b) MIOperator(device CSR of A') first %8.3f, then %s   ingest stage (checks, status read-back) %s" % (tc1[0], fmt(tc), fmt(sc)))
            lines.append("        adjoint / csr %.2f (cached pattern, medians)" % (np.median(ta) / np.median(tc)))
            ps = eu.MIOperator(At, ctx_s)
            adj = ps.adjoint()
            vals = torch.as_tensor(Mt.data).cuda()
            torch.cuda.synchronize()
            ra = by_events(lambda: adj.refresh(ps), S, 3, 20)
            rb = by_events(lambda: adj.update_values(vals), S, 3, 20)
            lines.append("    (c) device events: adj.refresh(parent) %s, adj.update_values(values) %s" % (fmt(ra), fmt(rb)))
            print("\n".join(lines[-6:]), flush=True)
            del parent, ps, adj, At, AHt, vals
    for T in (np.float64, np.complex128):
        rng = np.random.default_rng(9)
        D = torch.as_tensor((rng.standard_normal((nd, nd)) + (1j * rng.standard_normal((nd, nd)) if np.dtype(T).kind == "c" else 0)).astype(T)).cuda().t()
        torch.cuda.synchronize()
        parent = eu.MIOperator(D, ctx)
        ta, _, op = timed_dense(lambda c: parent.adjoint(), ctx, 3, 10)
        op = None
        tt = by_events(lambda: torch.conj_physical(D).contiguous(), torch.cuda.current_stream(), 3, 10)
        P = torch.conj_physical(D).contiguous().t()
        torch.cuda.synchronize()
        tc, _, opc = timed_dense(lambda c: eu.MIOperator(P, c), ctx, 3, 10)
        opc = None
        ps = eu.MIOperator(D, ctx_s)
        adj = ps.adjoint()
        ra = by_events(lambda: adj.refresh(ps), S, 3, 20)
        lines.append("dense %s, n = %d" % (np.dtype(T).name, nd))
        lines.append("    (a) parent.adjoint() %s" % fmt(ta))
        lines.append("    (b) MIOperator(packed device tensor of A') %s   torch's conj-transpose copy (device events) %s" % (fmt(tc), fmt(tt)))
        lines.append("    (c) device events: adj.refresh(parent) %s" % fmt(ra))
        print("\n".join(lines[-4:]), flush=True)
        del parent, ps, adj, D, P
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


def timed_dense(make, ctx, warm, reps):
    ts, op = [], None
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
    return np.array(ts), None, op


if __name__ == "__main__":
    main()
