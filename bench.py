"""bench.py -- headline benchmark: expv matvecs/s on BASELINE config 2
(n = 1e6, 5-diagonal non-symmetric sparse fp64, m = 30, t = 1.0; SURVEY.md §8d inputs).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one full expv(t, A, b): firststep + 30 Krylov steps (operator apply + orthogonalisation +
normalisation) + host Pade of the 30x30 Hessenberg + the beta*V*coef combine, with A, b and w resident in HBM.
One unit of the metric = one Krylov step ("matvec"), so an expv at m = 30 is 30 units.  Every rank runs its own
independent (A, b) problem (weak scaling, no data-path collective); value = N * K * 30 / max-over-ranks wall time.

A plain run sets up, warms up, times the K steps and prints the result line, nothing else.  With --full the same JSON
line also carries, measured in the same process on rank 0 at N = 1:
  value_cold    the K steps measured first in the process, before the device spin-up
  roofline      dominant kernel (the single-pass Krylov step): SURVEY §8d bytes per launch / mean launch time
  secondary     the other ways into the same path -- split API (arnoldi! + expv!), outputs complete on return (the
                C-ABI default), the Lanczos variant, config 4 (kiops, complex) and config 5 on one GPU
  cpu_baseline  the plain-C restatement of the reference loop on the host cores: all threads, one thread, and
                scipy's expm_multiply (a different algorithm, labelled as such)

--dump-outputs DIR writes what the last timed step returned to its caller as DIR/<name>.npy (rank 0; float64, or
float32 for a 32-bit path), so that two builds can be compared output for output: the inputs are seeded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_ROWS = 1_000_000
M_KRYLOV = 30
T_FINAL = 1.0
HBM_PEAK_GBS = 8000.0
C2_OFFSETS = (-2, -1, 0, 1, 2)
C2_VALS = (0.3, 1.2, -2.0, 0.8, -0.1)          # non-symmetric  -> Arnoldi path   
C2_SYM_VALS = (0.5, 1.0, -3.0, 1.0, 0.5)       # symmetric      -> Lanczos path


LINE_LIMIT = 4000     # the driver keeps the tail of stdout: the LAST line must fit (<= 4 KB)
DUMP_LIMIT = 64 << 20  # --dump-outputs: bytes in all


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per array (torch tensors are copied to the host), float32 stays float32, every
    other real type is written as float64.  The caller keeps the total within DUMP_LIMIT (a seeded sample of a larger output)."""
    os.makedirs(dirname, exist_ok=True)
    host = {}
    for name, a in arrays.items():
        a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
        if np.iscomplexobj(a):
            raise TypeError("--dump-outputs: %s is complex" % name)
        host[name] = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d byte limit" % (total, DUMP_LIMIT))
    for name, a in host.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def sample_columns(W, seed=2024):
    """A fixed, seeded sample of the columns of an n x ncols result that fits DUMP_LIMIT (all of them when they fit):
    returns (W[:, cols], cols)."""
    n, ncols = W.shape
    keep = max(1, min(ncols, DUMP_LIMIT // 2 // (8 * n)))
    cols = np.arange(ncols) if keep == ncols else np.sort(np.random.default_rng(seed).choice(ncols, size=keep, replace=False))
    return W[:, cols.tolist()], cols


def _r(x, sig=9):
    """floats to `sig` significant digits (value / ms_per_step stay consistent to 1e-8), containers recursively"""
    if isinstance(x, float):
        return float("%.*g" % (sig, x)) if np.isfinite(x) else None
    if isinstance(x, (np.floating,)):
        return _r(float(x), sig)
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def compact_line(out):
    """The one line the driver parses: headline keys, a flat config, a flat roofline, a flat cpu_baseline.  Everything else
    (per-kernel tables, the secondary entries with their prose) goes to bench_full.json and, in pieces, to stderr."""
    head = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data")
    c = {k: out[k] for k in head if k in out}
    cfg = {}
    for k, v in (out.get("config") or {}).items():
        if isinstance(v, str):
            cfg[k] = v if len(v) <= 240 else v[:237] + "..."
        elif isinstance(v, (int, float, bool, type(None), np.integer, np.floating)):
            cfg[k] = v
        elif k == "path" and isinstance(v, (list, tuple)):
            cfg[k] = list(v)
        elif k == "split_api_sync_outputs" and isinstance(v, dict):
            cfg[k] = {q: v.get(q) for q in ("value", "frac", "ms_per_call")}
        elif k == "secondary_fracs" and isinstance(v, dict):
            cfg[k] = {q: (float("%.3g" % z) if isinstance(z, float) else z) for q, z in v.items()}
        elif k == "secondary_fracs_minmax" and isinstance(v, dict):
            cfg[k] = v
        elif k == "reordered_setup_s" and isinstance(v, dict):      # {entry: [first creation, the same pattern again]} in seconds
            cfg[k] = v
    c["config"] = cfg
    for k in ("ranks_seen", "devices", "process_group", "standin"):
        if k in out:
            c[k] = out[k]
    if "per_rank_ms_per_step" in out:
        c["per_rank_ms_per_step"] = [float("%.5g" % v) for v in out["per_rank_ms_per_step"]]
    for k in ("gather", "verified", "collectives_per_call", "applications_per_call"):      # (c5 / c3 lines: small dicts / scalars)
        v = out.get(k)
        if isinstance(v, dict):
            c[k] = {q: z for q, z in v.items() if isinstance(z, (int, float, bool, type(None))) or (isinstance(z, str) and len(z) <= 80)}
        elif v is not None:
            c[k] = v
    r = out.get("roofline")
    if isinstance(r, dict):
        rr = {k: r.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "avg_launch_ms",
                                    "alg_bytes_per_launch", "expv_frac") if k in r}
        if isinstance(rr.get("traffic_source"), str) and len(rr["traffic_source"]) > 80:
            rr["traffic_source"] = rr["traffic_source"][:77] + "..."
        if isinstance(r.get("serial"), dict):
            rr["serial"] = {k: r["serial"].get(k) for k in ("frac", "avg_launch_ms")}
        c["roofline"] = rr
    b = out.get("cpu_baseline")
    if isinstance(b, dict):
        bb = {k: b.get(k) for k in ("value", "unit", "cores", "kind", "sample") if k in b}
        if isinstance(bb.get("sample"), str) and len(bb["sample"]) > 120:
            bb["sample"] = bb["sample"][:117] + "..."
        if "parity_rel_err_w" in b:
            bb["parity"] = b["parity_rel_err_w"]
        if isinstance(b.get("one_thread"), dict):
            bb["one_thread"] = {"value": b["one_thread"].get("value")}
        if isinstance(b.get("by_threads"), dict):
            bb["by_threads"] = {k: float("%.4g" % v) for k, v in b["by_threads"].items()}
        c["cpu_baseline"] = bb
    c["full"] = "bench_full.json"
    c = _r(c)
    line = json.dumps(c, separators=(",", ":"))
    # belt and braces: shed the optional parts, least important first, until the line fits
    for victim in (("config", "secondary_fracs_minmax"), ("per_rank_ms_per_step",), ("devices",), ("cpu_baseline", "by_threads"),
                   ("config", "path"), ("config", "secondary_fracs")):
        if len(line) <= LINE_LIMIT:
            break
        d = c
        for k in victim[:-1]:
            d = d.get(k, {})
        d.pop(victim[-1], None)
        line = json.dumps(c, separators=(",", ":"))
    if len(line) > LINE_LIMIT:
        raise SystemExit("bench.py: the result line is %d characters (limit %d): the driver could not parse it" % (len(line), LINE_LIMIT))
    return line


def emit(out):
    """full record -> bench_full.json (+ gpurun_out/ when present) and 'FULL[i] ' pieces on stderr; the compact record is the LAST (and only
    large) stdout line"""
    full = json.dumps(_r(out, 12))
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, "bench_full.json"), "w") as f:
                    f.write(full + "\n")
        except OSError:
            pass
    # (stdout carries the compact line and nothing else of this size: the full record goes to stderr, in pieces no reader chokes on)
    for i in range(0, len(full), 3000):
        print("FULL[%d] %s" % (i // 3000, full[i:i + 3000]), file=sys.stderr, flush=True)
    print(compact_line(out), flush=True)


def c2_operator(n, sym=False, dtype=np.float64):
    """constant diagonals at offsets (-2..2)."""
    import scipy.sparse as sp
    vals = C2_SYM_VALS if sym else C2_VALS
    diags = [np.full(n - abs(o), v, dtype=dtype) for o, v in zip(C2_OFFSETS, vals)]
    return sp.diags(diags, C2_OFFSETS, shape=(n, n), format="csr", dtype=dtype)


def general_sparse_operator(kind, n, seed=11):
    """Non-banded test operators of the secondary lines (the reference's own GPU test uses sprand, test/gpu/gputests.jl:41-58):
      "random"    regular rows: the diagonal + 4 entries in uniformly random columns (no locality at all: every gather of the
                  operator apply is a cache miss in an 8 MB vector);
      "local"     the same with the columns within +-2 % of the row, "local_narrow" within +-0.2 % (what a bandwidth-reducing
                  ordering of a 3-D / 2-D mesh of 1e6 nodes gives: bandwidth ~ n^(2/3) / n^(1/2));
      "powerlaw"  irregular rows: Zipf-distributed lengths (median 2, mean ~6, longest several hundred), random columns."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    if kind in ("random", "local", "local_narrow"):
        rows = np.repeat(np.arange(n), 4)
        reach = n // 50 if kind == "local" else n // 500
        cols = rng.integers(0, n, size=4 * n) if kind == "random" else np.clip(rows + rng.integers(-reach, reach + 1, size=4 * n), 0, n - 1)
        vals = rng.standard_normal(4 * n) * 0.3
    elif kind == "powerlaw":
        ln = np.minimum(rng.zipf(1.8, size=n), 2000)
        ln = np.minimum(np.maximum(1, (ln * (5.0 / ln.mean())).astype(np.int64)), 4000)
        rows = np.repeat(np.arange(n), ln)
        cols = rng.integers(0, n, size=rows.size)
        vals = rng.standard_normal(rows.size) / np.sqrt(np.repeat(ln, ln))
    else:
        raise ValueError(kind)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr() + sp.diags([np.full(n, -0.5)], [0], format="csr")
    A.sum_duplicates()
    return A.tocsr()


# ---------------------------------------------------------------- SURVEY.md §8d byte contracts --------------
def a_bytes(n, nnz, s=8):
    """A_B = nnz (s + 4) + 4 (n + 1): CSR with 32-bit indices."""
    return nnz * (s + 4) + 4 * (n + 1)


def alg_bytes_expv(n, nnz, m, s=8):
    """Full Arnoldi expv: m A_B + s n (m(m+1)/2 + 3m + 3)."""
    return m * a_bytes(n, nnz, s) + s * n * (m * (m + 1) // 2 + 3 * m + 3)


def alg_bytes_expv_window(n, nnz, m, w, s=8):
    """Lanczos / iop = w: per step A_B + s n (w + 2); + first step 2 s n + combine s n (m + 1)."""
    return m * (a_bytes(n, nnz, s) + s * n * (w + 2)) + 2 * s * n + s * n * (m + 1)


def alg_bytes_step(n, nnz, m, s=8):
    """ONE Krylov step of full Arnoldi averaged over j = 1..m: A_B + s n (j + 2) (read x, read V_1..V_j once,
    write v_{j+1}) -- the per-launch figure of the single-pass step kernel (one launch = one unit)."""
    return a_bytes(n, nnz, s) + s * n * ((m + 1) / 2.0 + 2)


def alg_bytes_kiops(n, nnz, steps, accepted, j_acc, p=1, w=2, s=16):
    """Config 4: per Krylov step A_B + s n (w + 2) + s n p; per accepted sub-step s n (j + 1) for the update."""
    return steps * (a_bytes(n, nnz, s) + s * n * (w + 2) + s * n * p) + accepted * s * n * (j_acc + 1)


def alg_bytes_kernel(name, n, nnz, m, s=8):
    """Average algorithmic bytes of ONE launch of a kernel over the m steps of an expv."""
    a_b = a_bytes(n, nnz, s)
    avg_j = (m + 1) / 2.0
    return {
        "matvec": a_b + 2 * s * n,                 # read A, read x, write y
        "dots": s * n * (avg_j + 2),               # read V[:,1:j], y and v_j (Gram row)
        "update": s * n * (avg_j + 2),             # read V[:,1:j] and y, write y
        "scale": 2 * s * n,                        # read y, write v_{j+1}
        "combine": s * n * (m + 1),                # read V[:,1:m], write w
        "firststep": 3 * s * n / 2.0,              # sumsq reads b; scale_copy reads b, writes v_1 (2 launches)
        "fused_a": a_b + s * n * (avg_j + 2),      # A + x + V[:,1:j-1] read, v_j and y written
        "fused_b": s * n * (avg_j + 2),
        "pipe_step": alg_bytes_step(n, nnz, m, s),
    }.get(name)


def pmc_traffic_file():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    return os.path.relpath(files[-1], ROOT) if files else None


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE
    collected in separate runs, gfx950 x2 read correction applied: tools/pmc_summary.py).  PMC collection
    cannot run inside this process, so the per-launch figure measured on the same command is read from
    profiles/; None when no pass has been recorded for this kernel."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if not files or kernel is None:
        return None
    data = json.load(open(files[-1]))
    key = {"fused_a": "k_fused_a", "fused_b": "k_update2", "dots": "k_dots", "update": "k_update<",
           "matvec": "k_spmv", "combine": "k_combine", "pipe_step": "k_pipe"}.get(kernel)
    if key is None:
        return None
    tot_b = tot_n = 0.0
    for name, v in data.items():
        if name.startswith(key) and "gate" not in name:
            tot_b += v["hbm_bytes_per_launch"] * v["launches"]
            tot_n += v["launches"]
    return (tot_b / tot_n) if tot_n else None


def load_dist_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mi_dist", os.path.join(ROOT, "exponentialutilities.jl_amd", "dist.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    return D


class Env:
    """Where the bench runs: device of the torch tensors, the process group, and how to wait for the device.
    The gloo CPU test (tests/test_dist_gloo.py) drives run_c5 with device="cpu" and a stand-in solver."""

    def __init__(self, torch, dist, world, rank, device, ctx, standin=None):
        self.torch, self.dist, self.world, self.rank, self.device, self.ctx = torch, dist, world, rank, device, ctx
        self.standin = standin          # name of the stand-in solver module (CPU plumbing tests only), or None
        # collectives run whenever a process group exists -- also at world size 1 under a launcher (torch.distributed.run
        # --nproc-per-node 1): the RCCL code path then executes for real on a one-GPU box
        self.coll = bool(dist is not None and dist.is_available() and dist.is_initialized())
        self.backend = dist.get_backend() if self.coll else None

    def sync(self):
        if str(self.device).startswith("cuda"):
            self.torch.cuda.synchronize()
        if self.ctx is not None:
            self.ctx.sync()

    def barrier(self):
        self.sync()
        if self.coll:
            self.dist.barrier()

    def ranks_seen(self):
        """all-reduce of ones: how many ranks really took part in the job."""
        if not self.coll:
            return 1
        t = self.torch.ones(1, dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return int(round(float(t.item())))

    def device_ids(self):
        """what every rank is bound to, in rank order: host + the GPU's uuid / PCI address (the stand-in: host + pid)."""
        import socket
        if str(self.device).startswith("cuda"):
            idx = self.torch.device(self.device).index or 0
            pr = self.torch.cuda.get_device_properties(idx)
            # uuid AND the PCI address: a driver that reports the same (or an all-zero) uuid for every GPU must not make N
            # properly bound ranks look like one device; two ranks on ONE device still agree in both and are refused
            pci = "pci-%s:%s.%s" % (getattr(pr, "pci_domain_id", "?"), getattr(pr, "pci_bus_id", "?"), getattr(pr, "pci_device_id", "?"))
            if pci == "pci-?:?.?":
                pci = "hip-%d" % idx        # (no PCI fields in this torch: the HIP ordinal of the device the rank is bound to)
            mine = "%s/%s/%s" % (socket.gethostname(), getattr(pr, "uuid", "no-uuid"), pci)
        else:
            mine = "%s/pid%d" % (socket.gethostname(), os.getpid())
        if not self.coll:
            return [mine]
        out = [None] * self.world
        self.dist.all_gather_object(out, mine)
        return out

    def check_ranks(self, want):
        """Fail loudly unless `want` ranks took part and every one of them is bound to its own device."""
        seen, ids = self.ranks_seen(), self.device_ids()
        if seen != want or len(set(ids)) != want:
            raise SystemExit("bench.py --gpus %d: %d rank(s) took part, bound to %d distinct device(s) %s -- refusing to report "
                             "a %d-GPU number" % (want, seen, len(set(ids)), ids, want))
        return seen, ids

    def per_rank(self, x):
        """every rank's value of a scalar, in rank order."""
        if not self.coll:
            return [float(x)]
        mine = self.torch.tensor([float(x)], dtype=self.torch.float64, device=self.device)
        out = self.torch.empty(self.world, dtype=self.torch.float64, device=self.device)
        self.dist.all_gather_into_tensor(out, mine)
        return [float(v) for v in out.cpu()]


def c5_problem(n, p, A0_data):
    """Problem p of config 5: C2 diagonals scaled by 1 + 0.1 rng(7).random()[p] and its own right-hand side; every rank
    can rebuild any problem (the round-end verification recomputes columns it does not own)."""
    scale = 1 + 0.1 * np.random.default_rng(7).random(p + 1)[p]
    return A0_data * scale, np.random.default_rng(1000 + p).standard_normal(n)


def c3_rows(torch, device, n, lo, hi, chunk=4096):
    """Rows [lo, hi) of the config-3 operator A = -2 I + randn(n, n) / sqrt(n), generated on the device block by block with a
    per-block seed, so any partition of the rows over ranks produces the same matrix.  Returned column-major."""
    rows = torch.empty((n, hi - lo), dtype=torch.float64, device=device).t()     # column-major (hi - lo) x n: the library's layout
    r = lo
    while r < hi:
        b0 = (r // chunk) * chunk                      # blocks are aligned to `chunk` rows of the GLOBAL matrix
        b1 = min(b0 + chunk, n)
        g = torch.Generator(device=device)
        g.manual_seed(40_000 + b0 // chunk)
        blk = torch.randn((b1 - b0, n), dtype=torch.float64, device=device, generator=g)
        blk.mul_(1.0 / np.sqrt(n))
        idx = torch.arange(b0, b1, device=device)
        blk[idx - b0, idx] -= 2.0
        e = min(b1, hi)
        rows[r - lo: e - lo].copy_(blk[r - b0: e - b0])
        r = e
        del blk
    return rows


def run_c3(args, eu, env, do_emit=True):
    """BASELINE configs[2]: phiv_timestep, adaptive, K = 4, dense fp64.  n = 2e5 (320 GB) does not fit one MI355X: with
    --gpus >= 2 the rows of A are sharded over the ranks (dist.RowShardedDense: local GEMV + one all-gather of the n-vector per
    operator application, the Krylov iteration replicated); at --gpus 1 the largest n that fits is used unless --n3 says
    otherwise.  Unit: operator applications (all mul! calls of the reference: p + m per sub-step + m per retry)."""
    torch, D = env.torch, load_dist_module()
    world, rank = env.world, env.rank
    seen, ids = env.check_ranks(world)
    n = args.n3 if args.n3 > 0 else (200_000 if world > 1 else 163_840)
    lo, hi = D.shard_range(n, world, rank)
    rows = c3_rows(torch, env.device, n, lo, hi)
    sh = D.RowShardedDense(rows, n, collective_at_world_1=env.coll)
    op = sh.operator(eu, env.ctx)
    g = torch.Generator(device=env.device)
    g.manual_seed(5)
    B = torch.randn((5, n), dtype=torch.float64, device=env.device, generator=g).t()      # K = 4: five coefficient columns
    st = {}

    def step():
        return eu.phiv_timestep(1.0, op, B, adaptive=True, tol=1e-7, m=10, stats=st)
    for _ in range(max(1, args.warmup)):
        u = step()
    env.barrier()
    a0, c0 = sh.applications, sh.collectives
    t0 = time.perf_counter()
    for _ in range(args.steps):
        u = step()
    env.barrier()
    elapsed_local = time.perf_counter() - t0
    if getattr(args, "dump_outputs", "") and rank == 0:
        dump_outputs(args.dump_outputs, {"u": u})
    apps = sh.applications - a0
    units, elapsed = D.aggregate_throughput(apps, elapsed_local, device=env.device)
    units /= world                                     # every rank counts the same (replicated) applications
    # every rank holds the full result of the replicated iteration: they must agree to the last bit
    chk = torch.stack([u.abs().sum(), (u * torch.arange(n, device=env.device, dtype=torch.float64)).sum()])
    lo_chk, hi_chk = chk.clone(), chk.clone()
    if env.coll:
        env.dist.all_reduce(lo_chk, op=env.dist.ReduceOp.MIN)
        env.dist.all_reduce(hi_chk, op=env.dist.ReduceOp.MAX)
    same = bool(torch.equal(lo_chk, hi_chk))
    bytes_per_app = 8.0 * n * n
    gbps_per_gpu = bytes_per_app * units / elapsed / 1e9 / world
    out = {"metric": "phiv_timestep operator applications/s, adaptive, K=4, dense fp64 n=%d" % n, "value": units / elapsed,
           "unit": "matvecs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic",
           "config": {"workload": "BASELINE configs[2]: phiv_timestep(1.0, A, B; adaptive, tol=1e-7, m0=10), dense A n=%d (%.1f GB), "
                                  "rows sharded over %d GPU(s)" % (n, 8e-9 * n * n, world), "n": n, "K": 4},
           "stats": {k: st.get(k) for k in ("num_timesteps", "matvecs", "m")}, "applications_per_call": apps / args.steps,
           "ranks_seen": seen, "devices": ids, "per_rank_ms_per_step": [1e3 * v / args.steps for v in env.per_rank(elapsed_local)],
           "process_group": env.backend, "collectives_per_call": (sh.collectives - c0) / args.steps,
           "verified": {"replicas_bitwise_equal": same},
           "roofline": {"bound": "hbm", "achieved": gbps_per_gpu, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbps_per_gpu / HBM_PEAK_GBS,
                        "traffic": None, "kernel": "k_gemv_dense on the rank's column-major row block (expv_mi_gemv_block) + all_gather of n*8 B",
                        "alg_bytes_per_launch": bytes_per_app / world}}
    if env.standin:
        out["standin"] = env.standin
        out["data"] = "stand-in solver on CPU (plumbing test of the launch / sharding / collective code: NOT a measurement)"
    if not same:
        raise SystemExit("config 3: the replicated iteration differs between ranks")
    if rank == 0 and do_emit:
        emit(out)
    return out


def run_c5(args, eu, env, n=100_000, m=M_KRYLOV, do_emit=True, dtype=np.float64):
    """BASELINE configs[4]: nprob independent expv problems (n = 1e5, C2 diagonals scaled per problem, m = 30), problems
    sharded over the ranks, one final gather of the results.  After the timed region two random columns
    of the gathered result are recomputed on this rank through the single-problem entry point and compared."""
    torch, D = env.torch, load_dist_module()
    nprob, world, rank = args.nprob, env.world, env.rank
    seen, ids = env.check_ranks(world)
    A0 = c2_operator(n).tocsr()
    A0.sort_indices()
    nnz = A0.nnz
    lo, hi = D.shard_range(nprob, world, rank)
    scales = 1 + 0.1 * np.random.default_rng(7).random(nprob)
    s_el = np.dtype(dtype).itemsize
    vals = torch.as_tensor(np.stack([A0.data * s for s in scales[lo:hi]]).astype(dtype), device=env.device)
    Bh = np.stack([np.random.default_rng(1000 + p).standard_normal(n) for p in range(lo, hi)]).astype(dtype)
    B = torch.as_tensor(Bh, device=env.device).t()

    local = {}

    def step():
        local["W"] = eu.expv_batch(T_FINAL, A0, vals, B, m=m, ctx=env.ctx)
        return D.gather_columns(local["W"], nprob) if env.coll else local["W"]

    for _ in range(args.warmup):
        step()
    env.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        W = step()
    env.barrier()
    elapsed_local = time.perf_counter() - t0
    if getattr(args, "dump_outputs", "") and rank == 0:       # (the gathered n x nprob result: a seeded sample of its columns)
        Ws, cols = sample_columns(W)
        dump_outputs(args.dump_outputs, {"W": Ws, "W_columns": cols})
    units, elapsed = D.aggregate_throughput((hi - lo) * m * args.steps, elapsed_local, device=env.device)
    # ---- the final gather alone (untimed extra): the one collective of the path, n x nprob fp64 over all ranks ----
    gather_ms = None
    if env.coll:
        env.barrier()
        tg = time.perf_counter()
        for _ in range(args.steps):
            D.gather_columns(local["W"], nprob)
        env.barrier()
        gather_ms = max(env.per_rank(1e3 * (time.perf_counter() - tg) / args.steps))
    # ---- verification (untimed): the gathered matrix against a rank-local recomputation of two random columns ----
    cols = sorted(set(int(c) for c in np.random.default_rng(4242 + rank).integers(0, nprob, size=2)))
    worst = 0.0
    for p in cols:
        data_p, b_p = c5_problem(n, p, A0.data)
        Ap = A0.copy()
        Ap.data = data_p.copy()
        ref = np.asarray(eu.expv(T_FINAL, Ap.astype(dtype), b_p.astype(dtype), m=m, ishermitian=False)).astype(np.float64)
        got = (W[:, p].cpu().numpy() if hasattr(W, "cpu") else np.asarray(W[:, p])).astype(np.float64)
        worst = max(worst, float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
    worst_all = max(env.per_rank(worst))
    b_alg = alg_bytes_expv(n, nnz, m, s=s_el) * nprob
    bar = 1e-12 if s_el == 8 else 2e-5
    per_gpu_gbps = b_alg / (elapsed / args.steps) / 1e9 / world
    out = {"metric": "expv matvecs/s, batch of independent problems n=%d sparse fp64 m=%d" % (n, m), "value": units / elapsed,
           "unit": "matvecs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": "f64" if s_el == 8 else "f32", "data": "synthetic",
           "config": {"workload": "BASELINE configs[4]: %d independent expv, n=%d, 5-diagonal, m=%d, sharded over %d "
                                  "GPU(s), final gather" % (nprob, n, m, world), "nprob": nprob, "n": n, "m": m},
           "ranks_seen": seen, "devices": ids, "per_rank_ms_per_step": [1e3 * v / args.steps for v in env.per_rank(elapsed_local)],
           "process_group": env.backend,
           "gather": {"ms": gather_ms, "bytes_total": 8.0 * n * nprob,
                      "what": "the final all_gather of the n x nprob result alone (inside ms_per_step too); null without a process group"},
           "verified": {"columns_per_rank": 2, "columns_rank0": cols, "max_rel_err": worst_all, "bar": bar,
                        "how": "gathered W[:, p] vs expv(t, A_p, b_p) recomputed on the checking rank"},
           "roofline": {"bound": "hbm", "achieved": per_gpu_gbps, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": per_gpu_gbps / HBM_PEAK_GBS, "traffic": None,
                        "note": "whole-call algorithmic GB/s per GPU (V of a problem is cache-resident)"}}
    if env.standin:
        out["standin"] = env.standin
        out["data"] = "stand-in solver on CPU (plumbing test of the launch / sharding / collective code: NOT a measurement)"
    if worst_all > bar:
        raise SystemExit("config 5: gathered result differs from the recomputed columns: %.3e" % worst_all)
    if rank == 0 and do_emit:
        emit(out)
    return out


# ---------------------------------------------------------------- secondary measurements (rank 0, N = 1) ----
def timed(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps


def timed_median(fn, steps, warmup, sync, batches=3):
    """Secondary entries with a few short calls: the median of `batches` timings of `steps` calls each -- one multi-millisecond
    stall of the host (a deferred free of an earlier entry's buffers, the OS) would otherwise BE the entry.  The headline keeps
    the contract's plain form (exactly K steps, one bracket)."""
    ts = sorted(timed(fn, steps, warmup if i == 0 else 0, sync) for i in range(batches))
    return ts[len(ts) // 2]


def timed_spread(fn, steps, warmup, sync, batches=3):
    """(median, min, max) seconds per call over `batches` timings of `steps` calls each"""
    ts = sorted(timed(fn, steps, warmup if i == 0 else 0, sync) for i in range(batches))
    return ts[len(ts) // 2], ts[0], ts[-1]


def secondary_block(args, eu, env, op, b, w, n, nnz, m):
    torch, ctx = env.torch, env.ctx
    sec = {}
    b_alg = alg_bytes_expv(n, nnz, m)

    def entry(what, sec_per_call, units_per_call, bytes_per_call, **extra):
        gbps = bytes_per_call / sec_per_call / 1e9
        e = {"what": what, "value": units_per_call / sec_per_call, "unit": "matvecs/s", "ms_per_call": 1e3 * sec_per_call,
             "alg_GB_per_call": bytes_per_call / 1e9, "alg_GBps": gbps, "frac": gbps / HBM_PEAK_GBS}
        e.update(extra)
        return e

    # (1) the two-call form of the reference: arnoldi!(Ks, A, b) then expv!(w, t, Ks)  -- what OrdinaryDiffEq calls
    Ks = eu.KrylovSubspace(np.float64, np.float64, n, m, 0, ctx)

    def split():
        eu.arnoldi_(Ks, op, b, m=m, ishermitian=False)
        eu.expv_(w, T_FINAL, Ks)
    sec["split_api"] = entry("arnoldi!(Ks,A,b) + expv!(w,t,Ks), C2 operator, stream-ordered outputs",
                             timed(split, args.steps, 2, env.sync), m, b_alg)
    # (2) outputs complete on return: the C-ABI default
    ctx.set_async_outputs(False)
    whole = lambda: eu.expv(T_FINAL, op, b, m=m, ishermitian=False, out=w)
    sec["sync_outputs"] = entry("expv(t,A,b), device result complete when the call returns (C-ABI default)",
                                timed(whole, args.steps, 2, env.sync), m, b_alg)
    # phiv(t, A, b, 4) = arnoldi! + phiv! with five output columns: the call of the non-adaptive exponential Runge-Kutta integrators
    ph4 = lambda: eu.phiv(T_FINAL, op, b, 4, m=m, ishermitian=False)
    ph4()
    env.sync()
    sec["phiv_k4"] = entry("phiv(t, A, b, 4): arnoldi! + phiv!, five output columns, results complete on return",
                           timed(ph4, args.steps, 2, env.sync), m, b_alg + 8 * n * 4)
    sec["split_api_sync_outputs"] = entry("arnoldi! + expv!, results complete on return",
                                          timed(split, args.steps, 2, env.sync), m, b_alg)
    ctx.set_async_outputs(True)
    del Ks
    # (3) Lanczos variant: symmetric 5-diagonal operator (SURVEY §8d secondary), window 2
    As = c2_operator(n, sym=True)
    ops = eu.MIOperator(As, ctx)
    lan = lambda: eu.expv(T_FINAL, ops, b, m=m, ishermitian=True, out=w)
    sec["lanczos"] = entry("expv, symmetric 5-diagonal operator (Lanczos, window 2), n=%d m=%d" % (n, m),
                           timed(lan, args.steps, 2, env.sync), m, alg_bytes_expv_window(n, As.nnz, m, 2))
    # (3a) the same call in the OPT-IN pipelined Lanczos mode (ortho = "pipelined": not the reference's arithmetic, include/expv_mi.h) -- same contract
    lanp = lambda: eu.expv(T_FINAL, ops, b, m=m, ishermitian=True, ortho="pipelined", out=w)
    lan()
    env.sync()
    w_lan = w.clone()
    lanp()
    env.sync()
    e = entry("expv, symmetric 5-diagonal operator, OPT-IN pipelined Lanczos recurrence (csrc/lanczos_pl.hip), n=%d m=%d" % (n, m),
              timed(lanp, args.steps, 2, env.sync), m, alg_bytes_expv_window(n, As.nnz, m, 2))
    e["path"] = list(eu.expv.last_stats["path"])
    e["rel_diff_to_default_path_result"] = float(torch.linalg.norm(w - w_lan) / torch.linalg.norm(w_lan))
    if "pipelined_lanczos" not in e["path"] or e["rel_diff_to_default_path_result"] > 1e-10:
        raise SystemExit("lanczos_pipelined: the mode did not run or disagrees with the default path: %r" % (e,))
    sec["lanczos_pipelined"] = e
    del w_lan
    # (3') the same symmetric operator through expv(...; mode = :error_estimate) (krylov_phiv_error_estimate.jl): Lanczos with the
    # a-posteriori stopping test after every step; unit = the Lanczos steps it took
    est = {}
    ee = lambda: eu.expv(T_FINAL, ops, b, m=m, mode="error_estimate", rtol=1e-8)
    ee()
    env.sync()
    tee = timed_median(ee, max(5, args.steps // 2), 1, env.sync)
    msteps = int(eu.expv.last_subspace.m)
    sec["error_estimate_mode"] = {"what": "expv(t, A, b; mode=:error_estimate, rtol=1e-8), symmetric 5-diagonal operator, n=%d, m <= %d" % (n, m),
                                  "value": msteps / tee, "unit": "matvecs/s", "ms_per_call": 1e3 * tee, "lanczos_steps": msteps}
    del ops, As
    # (3'') small systems (the size most exponential integrators run at): a Krylov step costs what its chain of dependent round trips
    # costs, whatever n: ms per expv and us per step
    small = {}
    for ns in (20_000, 100_000, 200_000):
        o_s = eu.MIOperator(c2_operator(ns), ctx)
        b_s, w_s = b[:ns].clone(), w[:ns].clone()
        f_s = lambda: eu.expv(T_FINAL, o_s, b_s, m=m, ishermitian=False, out=w_s)
        f_s()
        env.sync()
        t_s = timed_median(f_s, max(20, args.steps), 3, env.sync)
        small["n=%d" % ns] = {"ms_per_expv": 1e3 * t_s, "us_per_krylov_step": 1e6 * t_s / m, "matvecs_per_s": m / t_s}
        del o_s
    sec["small_systems"] = {"what": "expv, C2 operator at small n, m=%d: bound by the per-step reduction chain, not by bandwidth" % m, **small}
    # (3a) the headline operator with the "stencil" option: its diagonals are constant, so they can be passed as five scalars and
    # NOT streamed (40 MB less per step).  Reported separately: the headline measures the general path, which streams them.
    ctx.set_option("stencil", 1)
    sten = lambda: eu.expv(T_FINAL, op, b, m=m, ishermitian=False, out=w)
    sten()
    sec["constant_coefficient_stencil_option"] = entry(
        "expv, C2 operator with context option stencil=1: constant diagonals passed as scalars, operator values not streamed "
        "(the contract's A_B stays in the numerator; off by default, not the headline)", timed(sten, args.steps, 2, env.sync), m, b_alg)
    ctx.set_option("stencil", 0)
    # (3b) structured-grid operator: the same five values per row on the offsets of a 2-D 5-point stencil (-k, -1, 0, 1, k with
    # k = sqrt(n)): too wide for a halo recompute in its natural ordering.  Default (context option patch = 1, round 4): stored in a
    # grid-patch ordering at creation, the step runs in its PATCH form (a tile = a 16 x 32 patch of the grid, the ring of rows around
    # it recomputed); the key keeps its round-3 name.  Beside it the same operator in its natural ordering (patch = 0): the wave
    # form with per-tile flags, which is what this key measured up to round 3.
    import scipy.sparse as sp
    k = int(round(np.sqrt(n)))
    Ag = sp.diags([0.3, 1.2, -2.0, 0.8, -0.1], [-k, -1, 0, 1, k], shape=(n, n), format="csc")
    t_set = time.perf_counter()
    opg = eu.MIOperator(Ag, ctx)
    env.sync()
    t_set = time.perf_counter() - t_set
    grid = lambda: eu.expv(T_FINAL, opg, b, m=m, ishermitian=False, out=w)
    grid()
    e = entry("expv, 5-point grid stencil offsets (-%d,-1,0,1,%d), default options: grid-patch ordering at creation + patch form of the "
              "single-pass step (up to round 3: natural ordering + wave form), n=%d m=%d" % (k, k, n, m),
              timed(grid, args.steps, 2, env.sync), m, alg_bytes_expv(n, Ag.nnz, m))
    e["path"] = list(eu.expv.last_stats["path"])
    e["patch_info"] = opg.patch_info
    e["setup_s"] = t_set
    w_patch = w.clone()
    sec["grid_stencil_wave_form"] = e
    del opg
    ctx.set_option("patch", 0)
    t_set = time.perf_counter()
    opg = eu.MIOperator(Ag, ctx)
    env.sync()
    t_set = time.perf_counter() - t_set
    ctx.set_option("patch", 1)
    grid()
    e = entry("expv, the same grid stencil in its natural ordering (context option patch = 0): wave form of the single-pass step, "
              "n=%d m=%d" % (n, m), timed(grid, args.steps, 2, env.sync), m, alg_bytes_expv(n, Ag.nnz, m))
    e["path"] = list(eu.expv.last_stats["path"])
    e["setup_s"] = t_set
    e["rel_diff_patch_form_result"] = float(torch.linalg.norm(w_patch - w) / torch.linalg.norm(w))
    sec["grid_stencil_natural_ordering"] = e
    del opg, Ag, w_patch
    # (3b'') the 3-D counterpart: 7-point stencil on a k x k x k grid (offsets +-1, +-k, +-k^2, k = 100): the diagonals reach 20
    # tiles either way
    k3 = int(round(n ** (1.0 / 3.0)))
    n3d = k3 ** 3
    if n3d == n:
        Ag3 = sp.diags([0.2, 0.3, 1.1, -2.0, 0.7, -0.1, 0.15], [-k3 * k3, -k3, -1, 0, 1, k3, k3 * k3], shape=(n, n), format="csc")
        opg3 = eu.MIOperator(Ag3, ctx)
        grid3 = lambda: eu.expv(T_FINAL, opg3, b, m=m, ishermitian=False, out=w)
        grid3()
        e = entry("expv, 7-point grid stencil offsets (+-1, +-%d, +-%d) (wave form of the single-pass step), n=%d m=%d" % (k3, k3 * k3, n, m),
                  timed(grid3, args.steps, 2, env.sync), m, alg_bytes_expv(n, Ag3.nnz, m))
        e["path"] = list(eu.expv.last_stats["path"])
        sec["grid3d_stencil_wave_form"] = e
        del opg3, Ag3
    # (3b') the headline operator in Float32 (BlasFloat of the reference, ExponentialUtilities.jl:19): native 32-bit storage on
    # the single-pass step (4 rows per 16-byte pack, fp64 projection sums), priced against the s = 4 contract
    A32 = c2_operator(n).astype(np.float32)
    op32 = eu.MIOperator(A32, ctx)
    b32 = b.to(torch.float32)
    w32 = torch.empty(n, dtype=torch.float32, device=env.device)
    f32 = lambda: eu.expv(T_FINAL, op32, b32, m=m, ishermitian=False, out=w32)
    f32()
    env.sync()
    e = entry("expv, C2 operator in Float32 (native 32-bit storage, single-pass step), n=%d m=%d; contract with s = 4" % (n, m),
              timed(f32, args.steps, 2, env.sync), m, alg_bytes_expv(n, A32.nnz, m, s=4))
    e["path"] = list(eu.expv.last_stats["path"])
    eu.expv(T_FINAL, op, b, m=m, ishermitian=False, out=w)            # the fp64 result of the same problem
    env.sync()
    e["rel_diff_to_fp64_result"] = float(torch.linalg.norm(w32.double() - w) / torch.linalg.norm(w))
    sec["c2_float32"] = e
    del op32, A32
    # (3b''') the 2-D grid stencil in Float32: wave form on tiles of 1024 rows
    kg = int(round(np.sqrt(n)))
    Ag32 = sp.diags([0.3, 1.2, -2.0, 0.8, -0.1], [-kg, -1, 0, 1, kg], shape=(n, n), format="csc").astype(np.float32)
    opg32 = eu.MIOperator(Ag32, ctx)
    g32 = lambda: eu.expv(T_FINAL, opg32, b32, m=m, ishermitian=False, out=w32)
    g32()
    env.sync()
    e = entry("expv, 5-point grid stencil offsets (-%d,-1,0,1,%d) in Float32 (default: patch form, tiles of 1024 rows = 32 x 32 patches), n=%d m=%d; contract with s = 4" % (kg, kg, n, m),
              timed(g32, args.steps, 2, env.sync), m, alg_bytes_expv(n, Ag32.nnz, m, s=4))
    e["path"] = list(eu.expv.last_stats["path"])
    sec["grid_stencil_float32"] = e
    del opg32, Ag32
    # (3b4) a banded operator WITHOUT a diagonal form: ten distinct offsets within +-8 (more than the 8 diagonals the DIA form holds).  Up to
    # round 3 (and with patch = 0): halo form on SELL slots, 4 bytes of column index per entry from HBM; round 4: the patch form with the
    # halo as its ring and tile-local column indices whose equal blocks are stored once
    offs10 = [-8, -6, -5, -3, -1, 0, 1, 2, 4, 7]
    rg10 = np.random.default_rng(23)
    A10 = sp.diags([(0.1 + 0.05 * rg10.random(n - abs(o))) * (1 if o else -6.0) for o in offs10], offs10, shape=(n, n), format="csr")
    for key10, patch10 in (("banded_ten_offsets", 1), ("banded_ten_offsets_sell_halo", 0)):
        ctx.set_option("patch", patch10)
        op10 = eu.MIOperator(A10, ctx)
        ctx.set_option("patch", 1)
        f10 = lambda: eu.expv(T_FINAL, op10, b, m=m, ishermitian=False, out=w)
        f10()
        env.sync()
        e = entry("expv, banded operator with ten distinct offsets within +-8 (no diagonal form), context option patch = %d: %s, n=%d nnz=%d m=%d"
                  % (patch10, "tile-local columns (patch form, halo = ring)" if patch10 else "halo form on SELL slots", n, A10.nnz, m),
                  timed(f10, max(5, args.steps // 2), 1, env.sync), m, alg_bytes_expv(n, A10.nnz, m))
        e["path"] = list(eu.expv.last_stats["path"])
        sec[key10] = e
        del op10
    del A10
    # (3b4') a band of 40 rows: a thin 2-D grid (rows of 40 cells, offsets -40, -1, 0, 1, 40).  Too wide for the halo form; up to round 3
    # (and with patch = 0) the wave form; round 4: the patch form in the operator's own ordering (ring = the 80 rows around a tile)
    A40 = sp.diags([0.3, 1.2, -2.0, 0.8, -0.1], [-40, -1, 0, 1, 40], shape=(n, n), format="csr")
    for key40, patch40 in (("thin_grid_band40", 1), ("thin_grid_band40_wave_form", 0)):
        ctx.set_option("patch", patch40)
        op40 = eu.MIOperator(A40, ctx)
        ctx.set_option("patch", 1)
        f40 = lambda: eu.expv(T_FINAL, op40, b, m=m, ishermitian=False, out=w)
        f40()
        env.sync()
        e = entry("expv, thin 2-D grid: offsets (-40,-1,0,1,40), a band of 40 rows, context option patch = %d: %s, n=%d m=%d"
                  % (patch40, "patch form in the operator's own ordering" if patch40 else "wave form", n, m),
                  timed(f40, max(5, args.steps // 2), 1, env.sync), m, alg_bytes_expv(n, A40.nnz, m))
        e["path"] = list(eu.expv.last_stats["path"])
        sec[key40] = e
        del op40
    del A40
    # (3b5) a Schroedinger-type problem: real symmetric 5-point grid operator + potential, COMPLEX vector, imaginary time -- the Krylov
    # quantities are ComplexF64 (T = promote(eltype A, eltype b), arnoldi.jl:163), the iteration is Lanczos with complex t
    # (krylov_phiv.jl:252-280).  Round 4: patch form for the complex element types (tiles of 256 rows = 16 x 16 patches); before (and
    # with patch = 0): two-kernel step.  Contract: Lanczos, s = 16.
    ks_ = int(round(np.sqrt(n)))
    if ks_ * ks_ == n:
        rgs = np.random.default_rng(29)
        As_ = sp.diags([np.full(n - ks_, 1.0), np.full(n - 1, 1.0), -4.0 + 0.3 * rgs.random(n), np.full(n - 1, 1.0), np.full(n - ks_, 1.0)],
                       [-ks_, -1, 0, 1, ks_], shape=(n, n), format="csr").astype(np.complex128)
        bs_ = torch.as_tensor(rgs.standard_normal(n) + 1j * rgs.standard_normal(n), device=env.device)
        ws_ = torch.empty_like(bs_)
        ABs = As_.nnz * (16 + 4) + 4 * (n + 1)
        balg_s = m * (ABs + 16 * n * 4) + 16 * n * (m + 3)
        for keys_, patchs_ in (("schroedinger_grid_complex", 1), ("schroedinger_grid_complex_two_kernel", 0)):
            ctx.set_option("patch", patchs_)
            ops_ = eu.MIOperator(As_, ctx)
            ctx.set_option("patch", 1)
            fs_ = lambda: eu.expv(-0.6j, ops_, bs_, m=m, ishermitian=True, out=ws_)
            fs_()
            env.sync()
            e = entry("expv(-0.6im, A, b): real symmetric 5-point grid operator with a potential, complex vector (ComplexF64 Lanczos), patch = %d, n=%d m=%d; "
                      "contract: Lanczos with s = 16" % (patchs_, n, m), timed(fs_, max(5, args.steps // 2), 1, env.sync), m, balg_s)
            e["path"] = list(eu.expv.last_stats["path"])
            sec[keys_] = e
            del ops_
        del As_, bs_, ws_
    # (3c) general sparse operators: no band, no diagonals to exploit.  Regular rows with random columns and
    # with local columns, and irregular (power-law) rows; each result is checked against scipy's expm_multiply (a different
    # algorithm: converged regime, bar 1e-9), so a fast wrong answer cannot hide here.
    import scipy.sparse.linalg as spl
    for key, kind in (("general_sparse_random", "random"), ("general_sparse_local", "local"), ("general_sparse_local_narrow", "local_narrow"),
                      ("irregular_sparse_powerlaw", "powerlaw"), ("general_sparse_rcm", "shuffled_band"), ("general_sparse_rcm_grid", "shuffled_grid"),
                      ("general_sparse_mesh", "shuffled_trimesh")):
        if kind == "shuffled_band":
            # the headline operator under a random symmetric permutation of its unknowns (an "unstructured" numbering of a banded
            # problem): operator creation finds a bandwidth-reducing ordering (reverse Cuthill-McKee, reorder.h) and keeps P A P'
            q_ = np.random.default_rng(17).permutation(n)
            Ag = c2_operator(n)[q_][:, q_].tocsr()
        elif kind == "shuffled_grid":
            kq = int(round(np.sqrt(n)))
            q_ = np.random.default_rng(18).permutation(kq * kq)
            Ag = sp.diags([0.3, 1.2, -2.0, 0.8, -0.1], [-kq, -1, 0, 1, kq], shape=(kq * kq, kq * kq), format="csr")[q_][:, q_].tocsr()
            if kq * kq != n:
                continue
        elif kind == "shuffled_trimesh":
            # an "unstructured mesh": a triangulated planar k x k mesh (7 entries per row, no entries across the row ends of the
            # underlying grid, coefficients vary), numbered at random.  Creation cuts it into patches from breadth-first distances
            # (reorder.h: mesh_patches) -- the patch form of the single-pass step; with option patch = 0: RCM + wave form
            kq = int(round(np.sqrt(n)))
            if kq * kq != n:
                continue
            rg_ = np.random.default_rng(19)
            ii = np.arange(n)
            parts_ = []
            for dr, dc in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1)):
                r_, c_ = ii // kq + dr, ii % kq + dc
                ok_ = (r_ >= 0) & (r_ < kq) & (c_ >= 0) & (c_ < kq)
                v_ = (-2.0 if (dr, dc) == (0, 0) else 0.4) + 0.05 * rg_.random(n)
                parts_.append(sp.csr_matrix((v_[ok_], (ii[ok_], (r_ * kq + c_)[ok_])), shape=(n, n)))
            q_ = rg_.permutation(n)
            Ag = sum(parts_).tocsr()[q_][:, q_].tocsr()
        else:
            Ag = general_sparse_operator(kind, n)
        eu.plan_cache(clear=True)                      # (setup_s is the cost of a pattern never seen before)
        t0 = time.perf_counter()
        opx = eu.MIOperator(Ag, ctx)
        t_set = time.perf_counter() - t0
        t0 = time.perf_counter()
        opx_again = eu.MIOperator(Ag, ctx)             # the same pattern again: ordering / patch plan from the plan cache
        t_set_again = time.perf_counter() - t0
        del opx_again
        fx = lambda: eu.expv(T_FINAL, opx, b, m=m, ishermitian=False, out=w)
        fx()
        env.sync()
        pathx = list(eu.expv.last_stats["path"])
        wx = w.cpu().numpy().copy()
        tx = timed(fx, max(5, args.steps // 2), 1, env.sync)
        truth = spl.expm_multiply(Ag * T_FINAL, b.cpu().numpy())
        rl = np.diff(Ag.indptr)
        e = entry("expv, %s rows / %s columns, n=%d nnz=%d m=%d" % ("irregular (Zipf)" if kind == "powerlaw" else "regular",
                  {"local": "local (+-2 %% of the row)", "local_narrow": "local (+-0.2 %% of the row)",
                   "shuffled_band": "the C2 operator under a random symmetric permutation (reordered at creation)",
                   "shuffled_grid": "a 2-D 5-point grid operator under a random symmetric permutation (cut into patches at creation: patch form)",
                   "shuffled_trimesh": "a triangulated planar mesh numbered at random (cut into patches at creation: patch form)"}.get(kind, "uniformly random"), n, Ag.nnz, m),
                  tx, m, alg_bytes_expv(n, Ag.nnz, m),
                  path=pathx, setup_s=t_set, setup_again_s=t_set_again, row_len_max=int(rl.max()), row_len_mean=float(rl.mean()),
                  storage=eu.host_pattern_info(Ag)["path"], reorder=opx.reorder_info, patch_info=opx.patch_info,
                  verified_vs_scipy_expm_multiply=float(np.linalg.norm(wx - truth) / np.linalg.norm(truth)))
        if e["verified_vs_scipy_expm_multiply"] > 1e-9:
            raise SystemExit("%s: result differs from scipy's expm_multiply: %.3e" % (key, e["verified_vs_scipy_expm_multiply"]))
        sec[key] = e
        del opx, Ag
    # (4) BASELINE configs[3]: kiops, complex sparse, iop = 2 (the build's extension)
    Ac = (c2_operator(n) * (1 + 0.25j)).tocsc()
    opc = eu.MIOperator(Ac, ctx)
    rng = np.random.default_rng(6)
    uc = torch.as_tensor(rng.standard_normal(n) + 1j * rng.standard_normal(n), device=env.device)
    st_box = {}

    def kio():
        st_box["st"] = eu.kiops(1.0, opc, uc, allow_complex=True, ishermitian=False, opnorm=4.6)[1]
    kio()
    env.sync()
    c0 = ctx.counters()
    tk, tk_min, tk_max = timed_spread(kio, args.steps, 1, env.sync)       # (three batches: the entry moved by > 3 % between runs of one build)
    c1 = ctx.counters()
    steps_per_call = (c1["krylov_steps"] - c0["krylov_steps"]) / (3 * args.steps + 1)
    accepted, exps = st_box["st"][0], st_box["st"][3]
    # Krylov dimension at an accepted sub-step: every continuation after a rejection redoes one step (arnoldi.jl:368 loops
    # from `init`), so steps = sum_j(accepted) + (factorisations - accepted)
    j_acc = (steps_per_call - (exps - accepted)) / max(accepted, 1)
    # Units of the contract (B_alg is the REFERENCE algorithm's compulsory traffic, "regardless of the bytes the implementation
    # actually moves"): the reference recomputes step j after every rejected sub-step (`for j in init:m`, arnoldi.jl:368) -- the library
    # continues behind it (option kiops_skip_redo) and reaches the same H, V, w with one launch less per rejection.  ref_steps = what
    # the reference executes for this call; the device's own count and the fraction on that count are reported beside it.
    rejected = st_box["st"][1]
    ref_steps = steps_per_call + (rejected if ctx.get_option("kiops_skip_redo") else 0)
    j_acc = (ref_steps - (exps - accepted)) / max(accepted, 1)
    kb = alg_bytes_kiops(n, Ac.nnz, ref_steps, accepted, j_acc)
    e = entry("BASELINE configs[3]: kiops(1.0, A, u), n=%d complex-fp64 5-diagonal, iop=2, tol=1e-7 (complex = extension); units = Krylov steps of "
              "the reference's algorithm for this call (it recomputes one step per rejected sub-step, the library does not)" % n,
              tk, ref_steps, kb, stats=list(st_box["st"]), krylov_steps_per_call=ref_steps, device_krylov_steps_per_call=steps_per_call)
    e["unit"] = "Krylov steps/s"
    e["frac_min_max"] = [e["frac"] * tk / tk_max, e["frac"] * tk / tk_min]
    j_dev = (steps_per_call - (exps - accepted - rejected)) / max(accepted, 1) if ctx.get_option("kiops_skip_redo") else j_acc
    e["frac_counting_device_steps"] = alg_bytes_kiops(n, Ac.nnz, steps_per_call, accepted, j_dev) / tk / 1e9 / HBM_PEAK_GBS
    sec["c4_kiops_complex"] = e
    # (4') the method the reference itself defines: kiops on REAL Float64 operands (kiops.jl:89), the headline operator
    st_r = {}

    def kior():
        st_r["st"] = eu.kiops(1.0, op, b, ishermitian=False, opnorm=4.4)[1]
    kior()
    env.sync()
    c0 = ctx.counters()
    tkr = timed(kior, args.steps, 1, env.sync)
    c1 = ctx.counters()
    spc = (c1["krylov_steps"] - c0["krylov_steps"]) / (args.steps + 1)
    acc_r, exps_r = st_r["st"][0], st_r["st"][3]
    rej_r = st_r["st"][1]
    ref_spc = spc + (rej_r if ctx.get_option("kiops_skip_redo") else 0)      # (units of the reference's algorithm, as for C4)
    j_acc_r = (ref_spc - (exps_r - acc_r)) / max(acc_r, 1)
    e = entry("kiops(1.0, A, u) on the REAL C2 operator (the reference's own method), n=%d, iop=2, tol=1e-7; units as for c4_kiops_complex" % n, tkr, ref_spc,
              alg_bytes_kiops(n, nnz, ref_spc, acc_r, j_acc_r, s=8), stats=list(st_r["st"]), krylov_steps_per_call=ref_spc, device_krylov_steps_per_call=spc)
    e["unit"] = "Krylov steps/s"
    j_dev_r = (spc - (exps_r - acc_r - rej_r)) / max(acc_r, 1) if ctx.get_option("kiops_skip_redo") else j_acc_r
    e["frac_counting_device_steps"] = alg_bytes_kiops(n, nnz, spc, acc_r, j_dev_r, s=8) / tkr / 1e9 / HBM_PEAK_GBS
    sec["kiops_real"] = e
    # (4b) full Arnoldi on a COMPLEX operator at the default m = 30 (windows up to 29 + the closing pass's 30 columns): the C2
    # pattern x (1 + 0.25i), complex b -- the shape of the reference's own GPU test (test/gpu/gputests.jl:41-58: ComplexF64 operator,
    # expv(t, A_gpu, b) at default m).  Up to round 4 the single-pass step took complex windows <= 15, so this ran the two-kernel
    # step throughout.  Contract with s = 16.
    wc_ = torch.empty_like(uc)
    fca = lambda: eu.expv(T_FINAL, opc, uc, m=m, ishermitian=False, out=wc_)
    fca()
    env.sync()
    e = entry("expv(1.0, A, b), C2 pattern x (1+0.25i), ComplexF64, complex b, full Arnoldi m=%d, n=%d; contract with s = 16" % (m, n),
              timed(fca, max(5, args.steps // 2), 1, env.sync), m, alg_bytes_expv(n, Ac.nnz, m, s=16))
    e["path"] = list(eu.expv.last_stats["path"])
    sec["c2_complex_full_arnoldi"] = e
    del wc_
    del opc, Ac, uc
    # (4c) the reference's GPU test operator itself, scaled up: A = triu(sprand(ComplexF64, n, n, 10/n), 1) + sprand(ComplexF64, n, n,
    # 1/n), b = rand(ComplexF64, n), t = 0.1 (gputests.jl:41-52) -- uniformly random columns, no structure: the two-kernel step
    rgp = np.random.default_rng(41)
    nz1, nz2 = 10 * n, n
    r1, c1_ = rgp.integers(0, n, nz1), rgp.integers(0, n, nz1)
    keep = c1_ > r1
    Agp = (sp.csr_matrix(((rgp.random(nz1) + 1j * rgp.random(nz1))[keep], (r1[keep], c1_[keep])), shape=(n, n))
           + sp.csr_matrix((rgp.random(nz2) + 1j * rgp.random(nz2), (rgp.integers(0, n, nz2), rgp.integers(0, n, nz2))), shape=(n, n))).tocsr()
    Agp.sum_duplicates()
    opgp = eu.MIOperator(Agp, ctx)
    bgp = torch.as_tensor(rgp.random(n) + 1j * rgp.random(n), device=env.device)
    wgp = torch.empty_like(bgp)
    fgp = lambda: eu.expv(0.1, opgp, bgp, m=m, ishermitian=False, out=wgp)
    fgp()
    env.sync()
    e = entry("expv(0.1, A, b), the operator of the reference's GPU test (triu(sprand(ComplexF64, n, n, 10/n), 1) + sprand(ComplexF64, n, n, 1/n)) "
              "at n=%d, nnz=%d, m=%d; contract with s = 16" % (n, Agp.nnz, m),
              timed(fgp, max(3, args.steps // 4), 1, env.sync), m, alg_bytes_expv(n, Agp.nnz, m, s=16))
    e["path"] = list(eu.expv.last_stats["path"])
    sec["sprand_complex_gputests_shape"] = e
    del opgp, Agp, bgp, wgp
    # (4d) the reference's operator contract (docs/src/interfaces.md:7-36, basictests.jl:786-816): a matrix-free operator, mul! = a
    # callback on the library's stream.  Modular step: the window is read twice, extra launches; contract = the stored operator's
    # (the callback is a stencil function, the usual shape of a matrix-free Jacobian: y = sum_d c_d * shift(x, d) in six torch
    #  elementwise launches -- torch's own sparse-CSR product takes 3.3 ms per application on this device and would BE the entry)
    def stencil_mul(x):
        y = x * C2_VALS[2]
        for off, cv in zip(C2_OFFSETS, C2_VALS):
            if off < 0:
                y[-off:].add_(x[:off], alpha=cv)
            elif off > 0:
                y[:-off].add_(x[off:], alpha=cv)
        return y
    # (the callback is LINEAR: it opts in to the two-kernel step, context option matfree_fused = 1; the default since round 6 is the
    #  reference's contract -- mul! on the normalised column, modular launches)
    ctx.set_option("matfree_fused", 1)
    mf_ = eu.MIOperator(None, ctx, matvec=stencil_mul, shape=(n, n), dtype=np.float64, ishermitian=False)
    fmf = lambda: eu.expv(T_FINAL, mf_, b, m=m, ishermitian=False, out=w)
    eu.expv(T_FINAL, op, b, m=m, ishermitian=False, out=w)
    env.sync()
    w_stored = w.clone()
    fmf()
    env.sync()
    e = entry("expv(1.0, A, b) through a matrix-free operator (callback: the C2 stencil as six torch elementwise launches), n=%d m=%d" % (n, m),
              timed(fmf, max(5, args.steps // 2), 1, env.sync), m, b_alg)
    e["path"] = list(eu.expv.last_stats["path"])
    e["rel_diff_to_stored_operator_result"] = float(torch.linalg.norm(w - w_stored) / torch.linalg.norm(w_stored))
    xm_ = torch.randn(n, dtype=torch.float64, device=env.device)
    e["callback_matvec_alone_us"] = 1e6 * timed(lambda: stencil_mul(xm_), 30, 5, env.sync)
    e["option"] = "matfree_fused = 1 (linear callback)"
    sec["matrix_free_callback"] = e
    env.sync()
    del mf_
    # (4e) the same operator as a COMPILED callback: one hand-written HIP kernel behind expv_mi_matvec_fn (tests/c_harness/stencil_callback.hip,
    # what a Julia host passes as a @cfunction) -- the library's own share of a matrix-free step, no Python inside the factorisation
    cb_so = os.path.join(ROOT, "tests", "c_harness", "libstencil_cb.so")
    if os.path.exists(cb_so):
        import ctypes as C_

        class StencilOp(C_.Structure):
            _fields_ = [("n", C_.c_int64), ("ndiag", C_.c_int), ("off", C_.c_int * 8), ("coef", C_.c_double * 8)]
        cbl = C_.CDLL(cb_so)
        cbl.stencil_matvec.argtypes = [C_.c_void_p] * 4
        cbl.stencil_matvec.restype = C_.c_int
        assert cbl.stencil_op_sizeof() == C_.sizeof(StencilOp)
        sop = StencilOp(n, len(C2_OFFSETS), (C_.c_int * 8)(*C2_OFFSETS), (C_.c_double * 8)(*C2_VALS))
        for fused_opt, key in ((1, "matrix_free_compiled"), (0, "matrix_free_compiled_default_path")):
            ctx.set_option("matfree_fused", fused_opt)
            mfc = eu.MIOperator(None, ctx, matvec_c=(cbl.stencil_matvec, C_.addressof(sop)), shape=(n, n), dtype=np.float64, ishermitian=False)
            fmc = lambda: eu.expv(T_FINAL, mfc, b, m=m, ishermitian=False, out=w)
            fmc()
            env.sync()
            e = entry("expv(1.0, A, b) through a COMPILED matrix-free operator (callback = one HIP kernel, tests/c_harness/stencil_callback.hip), "
                      "n=%d m=%d, option matfree_fused = %d%s" % (n, m, fused_opt, "" if fused_opt else " (the default: mul! on the normalised column, modular launches)"),
                      timed(fmc, max(5, args.steps // 2), 1, env.sync), m, b_alg)
            e["path"] = list(eu.expv.last_stats["path"])
            e["rel_diff_to_stored_operator_result"] = float(torch.linalg.norm(w - w_stored) / torch.linalg.norm(w_stored))
            if e["rel_diff_to_stored_operator_result"] > 1e-10:
                raise SystemExit("%s: result differs from the stored operator's: %.3e" % (key, e["rel_diff_to_stored_operator_result"]))
            ym_ = torch.empty_like(xm_)
            st_ = torch.cuda.current_stream().cuda_stream
            e["callback_matvec_alone_us"] = 1e6 * timed(lambda: cbl.stencil_matvec(C_.addressof(sop), C_.c_void_p(xm_.data_ptr()), C_.c_void_p(ym_.data_ptr()), C_.c_void_p(st_)), 30, 5, env.sync)
            sec[key] = e
            env.sync()
            del mfc
    ctx.set_option("matfree_fused", 0)
    del w_stored, xm_
    # (5) BASELINE configs[4] on ONE GPU: its 1/8 share of the 1024 problems
    a5 = argparse.Namespace(nprob=128, steps=max(2, args.steps // 5), warmup=1)
    o5s = sorted((run_c5(a5, eu, env, do_emit=False) for _ in range(5)), key=lambda o_: o_["roofline"]["frac"])      # five runs: median, spread
    o5 = o5s[2]
    sec["c5_one_gpu_share"] = {"what": "BASELINE configs[4], one GPU's share: 128 independent expv, n=1e5, m=30 (median of five runs)",
                               "value": o5["value"], "unit": "matvecs/s", "ms_per_call": o5["ms_per_step"],
                               "alg_GBps": o5["roofline"]["achieved"], "frac": o5["roofline"]["frac"],
                               "frac_min_max": [o5s[0]["roofline"]["frac"], o5s[-1]["roofline"]["frac"]],
                               "verified_max_rel_err": max(o_["verified"]["max_rel_err"] for o_ in o5s)}
    # (5a) the same share in Float32 (BlasFloat, ExponentialUtilities.jl:19): batched single-pass step on 32-bit storage
    a5f = argparse.Namespace(nprob=128, steps=max(2, args.steps // 5), warmup=1)
    o5f = run_c5(a5f, eu, env, do_emit=False, dtype=np.float32)
    sec["c5_float32"] = {"what": "BASELINE configs[4] in Float32, one GPU's share: 128 independent expv, n=1e5, m=30; contract with s = 4",
                         "value": o5f["value"], "unit": "matvecs/s", "ms_per_call": o5f["ms_per_step"],
                         "alg_GBps": o5f["roofline"]["achieved"], "frac": o5f["roofline"]["frac"],
                         "verified_max_rel_err": o5f["verified"]["max_rel_err"]}
    # (5b) the integrator-facing calls on the headline operator (what OrdinaryDiffEq's exponential integrators call,
    # krylov_phiv_adaptive.jl:57-114, :184-232): adaptive expv_timestep and adaptive phiv_timestep with K = 4 phi-functions;
    # unit = operator applications (Krylov steps + the p applications of the W recurrence per sub-step)
    Bk = torch.as_tensor(np.random.default_rng(5).standard_normal((5, n)), device=env.device).t()      # n x 5, column-major
    for key, what, fn in (
            ("expv_timestep_adaptive", "expv_timestep([0.5, 1.0], A, b; adaptive=true, tol=1e-6), C2 operator",
             lambda st: eu.expv_timestep([0.5, 1.0], op, b, tol=1e-6, adaptive=True, stats=st)),
            ("phiv_timestep_K4_sparse", "phiv_timestep([1.0], A, B; adaptive=true, tol=1e-8), K=4 (B is n x 5), C2 operator",
             lambda st: eu.phiv_timestep([1.0], op, Bk, tol=1e-8, adaptive=True, stats=st))):
        stx = {}
        fn(stx)
        env.sync()
        c0 = ctx.counters()
        reps = max(5, args.steps // 2)
        tt = timed_median(lambda: fn(stx), reps, 1, env.sync)
        c1 = ctx.counters()
        ksteps = (c1["krylov_steps"] - c0["krylov_steps"]) / (reps + 1)
        apps = ksteps + (c1["op_applies"] - c0["op_applies"]) / (reps + 1)
        sec[key] = {"what": what, "value": apps / tt, "unit": "matvecs/s", "ms_per_call": 1e3 * tt, "krylov_steps_per_call": ksteps,
                    "operator_applications_per_call": apps, "us_per_operator_application": 1e6 * tt / max(apps, 1),
                    "stats": {k: stx.get(k) for k in ("num_timesteps", "matvecs", "m", "arnoldi_calls", "arnoldi_reused")}}
    # (6) BASELINE configs[2] on one GPU at a size that costs a few seconds: adaptive phiv_timestep, K = 4, dense fp64 operator
    # generated on the device (n = 65 536: 34 GB); the step is operator applications (mul!), the kernel the library's dense GEMV
    for n3, key3, reps3 in ((65_536, "c3_dense_phiv_timestep", 3), (163_840, "c3_dense_phiv_timestep_n163840", 2)):
        # (the second size is the LARGEST single-GPU configuration of BASELINE configs[2]: 214.7 GB of the 288 GB; generation ~15 s)
        if n3 > 65_536 and args.no_c3_full:
            continue
        try:
            A3 = c3_rows(torch, env.device, n3, 0, n3)
            op3 = eu.MIOperator(A3, ctx)                      # device-resident, column-major: no copy
            g3 = torch.Generator(device=env.device)
            g3.manual_seed(5)
            B3 = torch.randn((5, n3), dtype=torch.float64, device=env.device, generator=g3).t()
            st3 = {}
            f3 = lambda: eu.phiv_timestep(1.0, op3, B3, adaptive=True, tol=1e-7, m=10, stats=st3)
            f3()
            env.sync()
            ctx.prof_reset()
            ctx.prof_enable(True)
            c0 = ctx.counters()
            t3 = timed(f3, reps3, 0, env.sync)
            c1 = ctx.counters()
            pr3 = ctx.prof_get()
            ctx.prof_enable(False)
            apps = ((c1["op_applies"] - c0["op_applies"]) + (c1["krylov_steps"] - c0["krylov_steps"])) / reps3
            mv = pr3.get("matvec", {"launches": 0, "total_ms": 0.0})
            gemv_ms = mv["total_ms"] / max(mv["launches"], 1)
            sec[key3] = {
                "what": "BASELINE configs[2] at n=%d (%.1f GB, one GPU): phiv_timestep(1.0, A, B; adaptive, K=4, tol=1e-7, m0=10), dense fp64 A "
                        "generated on the device; unit = operator applications (all mul! calls)" % (n3, 8e-9 * n3 * n3),
                "value": apps / t3, "unit": "matvecs/s", "ms_per_call": 1e3 * t3, "applications_per_call": apps,
                "stats": {k: st3.get(k) for k in ("num_timesteps", "matvecs", "m")},
                "gemv_avg_ms": gemv_ms, "gemv_launches_profiled": mv["launches"],
                "gemv_alg_GBps": (8.0 * n3 * n3 / (gemv_ms * 1e-3) / 1e9) if gemv_ms > 0 else None,
                "frac": (8.0 * n3 * n3 / (gemv_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if gemv_ms > 0 else None,
                "whole_call_alg_GBps": 8.0 * n3 * n3 * apps / t3 / 1e9}
            del op3, A3, B3
            torch.cuda.empty_cache()
        except torch.cuda.OutOfMemoryError as ex:      # (a smaller card: say so instead of dropping the line silently)
            sec[key3] = {"error": "out of memory for the %d x %d operator: %s" % (n3, n3, str(ex)[:80])}
    return sec


def cpu_baseline_block(A, b_host, w_dev, m, n):
    """The reference loop (literal MGS) restated in plain C on the host cores: all threads, then ONE thread (the
    reference's SparseMatrixCSC mul! is single-threaded), and scipy's expm_multiply as a labelled extra."""
    from oracle import c_oracle as co
    threads = co.num_threads()

    def run(nthreads, budget_s, max_reps):
        co.set_num_threads(nthreads)
        reps, tc, wo, r = 0, 0.0, None, None
        t_start = time.perf_counter()
        while reps < max_reps and (time.perf_counter() - t_start) < budget_s:
            t1 = time.perf_counter()
            wo, r = co.expv_csr(T_FINAL, A, b_host, m=m)
            tc += time.perf_counter() - t1
            reps += 1
        return reps * r["m"] / tc, reps, wo

    # the box may grant this container fewer CPUs than it shows (cgroup quota): a ladder of thread counts, bounded, and the
    # best one is the baseline; every point is reported
    ladder = sorted(set(t for t in (1, 8, 16, 32, 64, threads) if t <= threads))
    points, wo = {}, None
    for t in ladder:
        v, reps, wo_t = run(t, 6.0, 2 if t > 1 else 1)
        points[t] = {"value": v, "reps": reps}
        wo = wo_t if wo is None else wo
    co.set_num_threads(threads)
    best = max(points, key=lambda t: points[t]["value"])
    err = float(np.linalg.norm(w_dev - wo) / np.linalg.norm(wo))
    out = {"value": points[best]["value"], "unit": "matvecs/s", "cores": best, "kind": "port",
           "sample": "%d full expv call(s) of the same workload (n=%d, m=%d) through oracle/expv_oracle.c at each of OpenMP "
                     "threads = %s; value = the best (threads = %d); host shows %d hardware threads"
                     % (points[best]["reps"], n, m, ladder, best, threads),
           "parity_rel_err_w": err,
           "by_threads": {str(t): points[t]["value"] for t in ladder},
           "one_thread": {"value": points[1]["value"], "unit": "matvecs/s", "cores": 1,
                          "sample": "%d full expv call(s), OMP threads = 1 (the reference's CSC mul! and BLAS-1 loop "
                                    "on this problem are single-threaded)" % points[1]["reps"]}}
    try:
        import scipy.sparse.linalg as spl
        t1 = time.perf_counter()
        we = spl.expm_multiply(A * T_FINAL, b_host)
        te = time.perf_counter() - t1
        out["scipy_expm_multiply"] = {"ms_per_call": 1e3 * te, "calls": 1,
                                      "label": "scipy.sparse.linalg.expm_multiply (Al-Mohy & Higham truncated Taylor: a "
                                               "DIFFERENT algorithm, shown for scale only)",
                                      "rel_diff_to_krylov_w": float(np.linalg.norm(we - wo) / np.linalg.norm(wo))}
    except Exception as e:  # pragma: no cover
        out["scipy_expm_multiply"] = {"error": repr(e)}
    return out


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(ngpus, argv):
    """`python bench.py --gpus N` with no launcher around it: start N ranks (one per GPU) of this same script under
    torch.distributed.run on this node and hand back its exit status.  Rendezvous on 127.0.0.1."""
    import subprocess
    argv = ["--rows" if a == "--n" else a for a in argv]     # (torch.distributed.run's own parser would claim a bare --n)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % ngpus,
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    envv = dict(os.environ)
    envv.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL across processes needs it on this driver
    envv.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=envv)      # (EXPV_MI_BENCH_STANDIN_OK, when a test set it, is inherited)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", "--rows", dest="n", type=int, default=N_ROWS, help="override problem size (debug only; invalidates the metric)")
    ap.add_argument("--ortho", default="auto", choices=["auto", "mgs", "lowsync"])
    ap.add_argument("--spinup", type=float, default=0.6, help="seconds of untimed calls before the warm-up steps (device clocks; 0 = none)")
    ap.add_argument("--full", action="store_true", help="c2: also the cold figure, the per-kernel roofline passes, the secondary "
                                                        "measurements and the CPU baseline (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the secondary measurements (split API, Lanczos, C4, C5)")
    ap.add_argument("--no-c3-full", action="store_true", help="--full, secondary block: skip BASELINE configs[2] at its largest single-GPU size (n = 163 840, 214.7 GB)")
    ap.add_argument("--no-serial-pass", action="store_true", help="--full: skip the extra non-overlapped profiling pass")
    ap.add_argument("--sync-outputs", action="store_true", help="every call returns only when its device result is complete")
    ap.add_argument("--split-api", action="store_true", help="time arnoldi!(Ks,A,b) + expv!(w,t,Ks) instead of expv(t,A,b)")
    ap.add_argument("--config", default="c2", choices=["c2", "c5", "c3"],
                    help="c2 (default, the headline metric), c5: batch of --nprob independent n=1e5 problems, or c3: adaptive "
                         "phiv_timestep on a dense operator whose rows are sharded over the ranks")
    ap.add_argument("--n3", type=int, default=0, help="c3: operator size (default 2e5 on >= 2 GPUs, 163840 on one)")
    ap.add_argument("--n5", type=int, default=100_000, help="c5: problem size (debug only)")
    ap.add_argument("--nprob", type=int, default=1024, help="c5: total number of problems over all GPUs")
    ap.add_argument("--standin", default="", help="TESTING ONLY: module with the product's Python signatures run on CPU tensors "
                                                  "under gloo (tests/standin_eu.py) -- exercises launch, sharding, collectives "
                                                  "and verification of this script without a GPU; its output is labelled and "
                                                  "is not a measurement")
    args = ap.parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: become the launcher (the driver's own form, torch.distributed.run, sets WORLD_SIZE)
        raise SystemExit(launch_ranks(args.gpus, argv))
    import torch
    import torch.distributed as dist

    launched = "WORLD_SIZE" in os.environ and "MASTER_PORT" in os.environ      # under torch.distributed.run (the driver's N > 1 form)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d started with WORLD_SIZE=%d: one rank per GPU is the contract" % (args.gpus, world))
    if args.standin:
        # the stand-in swaps the product for a CPU solver: only the gloo plumbing tests may do that, and they say so in the
        # environment as well -- a stray flag on a command line cannot put stand-in output into a bench line
        if os.environ.get("EXPV_MI_BENCH_STANDIN_OK") != "tests-only":
            raise SystemExit("--standin is test plumbing (tests/test_dist_gloo.py); refusing to run it as a benchmark")
        import importlib
        eu = importlib.import_module(args.standin).StandIn
        if launched:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
        env = Env(torch, dist, world, rank, "cpu", None, standin=args.standin)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
        if local_rank >= torch.cuda.device_count():
            raise SystemExit("rank %d wants GPU %d, the node shows %d" % (rank, local_rank, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        if launched:      # one rank per GPU over RCCL -- also a single rank under a launcher (the collectives then run at world size 1)
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        import expv_mi_loader
        eu = expv_mi_loader.load()
        # device-resident results are stream-ordered (like any HIP library); barrier() below syncs the context
        ctx = eu.Context(device=local_rank, async_outputs=not args.sync_outputs)
        env = Env(torch, dist, world, rank, torch.device("cuda", local_rank), ctx)
    try:
        if args.config == "c5":
            run_c5(args, eu, env, n=args.n5)
        elif args.config == "c3":
            run_c3(args, eu, env)
        else:
            run_c2(args, eu, env)
    finally:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()


def run_c2(args, eu, env):
    """BASELINE configs[1], the headline: one independent expv problem per rank (weak scaling, no data-path collective)."""
    torch, dist, ctx = env.torch, env.dist, env.ctx
    world, rank = env.world, env.rank
    seen, ids = env.check_ranks(world)
    n, m = args.n, M_KRYLOV
    A = c2_operator(n)
    nnz = A.nnz
    t_setup = time.perf_counter()
    op = eu.MIOperator(A, ctx)                      # CSR32 upload + properties: setup, not timed
    t_setup = time.perf_counter() - t_setup
    b_host = np.random.default_rng(3 + rank).standard_normal(n)
    b = torch.as_tensor(b_host, device=env.device)
    w = torch.empty(n, dtype=torch.float64, device=env.device)
    Ks = eu.KrylovSubspace(np.float64, np.float64, n, m, 0, ctx) if args.split_api else None

    def one_expv():
        if args.split_api:      # arnoldi!(Ks, A, b) then expv!(w, t, Ks): the two-call form of the reference
            eu.arnoldi_(Ks, op, b, m=m, ishermitian=False, ortho=args.ortho)
            eu.expv_(w, T_FINAL, Ks)
            return Ks.m
        eu.expv(T_FINAL, op, b, m=m, ishermitian=False, ortho=args.ortho, out=w)    # expv(t, A, b; m)
        return eu.expv.last_stats["m"]

    # device spin-up (untimed, before the W warm-up steps of the contract): a box that has just been handed over clocks up during
    # its first few hundred milliseconds of work -- the first run on a fresh box measured 3 % below the second (26.1 k vs 26.9 k)
    # ... and (--full) the figure WITHOUT that spin-up, measured first in the process (VERDICT r5 / ADVICE r5): the contract's W warm-up
    # steps, then the same K steps -- what the first calls of an ODE integrator see on a box that has been idle (`value_cold` in the line)
    cold = None
    if args.full and env.ctx is not None and args.spinup > 0:
        for _ in range(args.warmup):
            one_expv()
        env.barrier()
        tc0 = time.perf_counter()
        cu = 0
        for _ in range(args.steps):
            cu += one_expv()
        env.barrier()
        tc = max(env.per_rank(time.perf_counter() - tc0))
        cold = {"value": float(sum(env.per_rank(cu))) / tc, "ms_per_step": 1e3 * tc / args.steps}
    spin_t0, spin_calls = time.perf_counter(), 0
    while env.ctx is not None and time.perf_counter() - spin_t0 < args.spinup:
        one_expv()
        spin_calls += 1
        if spin_calls % 16 == 0:
            env.sync()
    for _ in range(args.warmup):
        one_expv()
    env.barrier()
    t0 = time.perf_counter()
    units = 0
    for _ in range(args.steps):
        units += one_expv()
    env.barrier()
    elapsed_local = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:                        # (before any later pass overwrites w)
        dump_outputs(args.dump_outputs, {"w": w})
    elapsed = max(env.per_rank(elapsed_local))                 # MAX over ranks
    units_total = float(sum(env.per_rank(units)))              # SUM over ranks
    value = units_total / elapsed
    ms_per_step = 1e3 * elapsed / args.steps
    per_rank_ms = [1e3 * v / args.steps for v in env.per_rank(elapsed_local)]
    path = list(getattr(eu.expv, "last_stats", {}).get("path", [])) if not args.split_api else None
    if world > 1:
        # every rank ran its own problem: their results must all be finite and different (distinct right-hand sides)
        chk = env.per_rank(float(w.abs().sum()))
        if not (all(np.isfinite(chk)) and len(set(chk)) == world):
            raise SystemExit("config 2 at %d ranks: per-rank results are not %d distinct finite vectors: %s" % (world, world, chk))

    # ---- (--full) per-kernel HIP-event timing of the same K steps (separate pass: events perturb the headline) ---
    prof = {}
    if args.full and ctx is not None:
        ctx.prof_reset()
        ctx.prof_enable(True)
        for _ in range(args.steps):
            one_expv()
        ctx.sync()
        prof = ctx.prof_get()
        ctx.prof_enable(False)
    # the single-pass pipeline records its step kernel under "fused_a" and has no per-step "fused_b"
    pipeline = "fused_a" in prof and prof.get("fused_b", {"launches": 0})["launches"] < prof["fused_a"]["launches"] / 2
    if pipeline:
        prof["pipe_step"] = prof.pop("fused_a")
    serial = None
    if pipeline and not args.no_serial_pass:
        # the default mode overlaps consecutive step kernels (two streams), so a kernel has no duration of its own:
        # "avg_ms" above is the factorisation span / steps.  One more pass with one launch after the other gives
        # per-launch HIP-event durations that a rocprofv3 --kernel-trace of the same mode reproduces.
        ctx.set_pipeline_overlap(False)
        for _ in range(2):
            one_expv()
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        t1 = time.perf_counter()
        for _ in range(args.steps):
            one_expv()
        ctx.sync()
        t_serial = (time.perf_counter() - t1) / args.steps
        ps = ctx.prof_get()
        ctx.prof_enable(False)
        ctx.set_pipeline_overlap(True)
        if "fused_a" in ps:
            avg = ps["fused_a"]["total_ms"] / ps["fused_a"]["launches"]
            ab = alg_bytes_kernel("pipe_step", n, nnz, m)
            serial = {"avg_launch_ms": avg, "alg_GBps": ab / (avg * 1e-3) / 1e9, "frac": ab / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "ms_per_expv": 1e3 * t_serial, "matvecs_per_s": m / t_serial}
    kern = {}
    for name, p in prof.items():
        ab = alg_bytes_kernel(name, n, nnz, m)
        avg_ms = p["total_ms"] / p["launches"]
        kern[name] = {"launches_per_expv": p["launches"] / args.steps, "avg_ms": avg_ms,
                      "total_ms_per_expv": p["total_ms"] / args.steps,
                      "alg_bytes_per_launch": ab,
                      "alg_GBps": (ab / (avg_ms * 1e-3) / 1e9) if ab else None}
    dom = max(kern, key=lambda k: kern[k]["total_ms_per_expv"]) if kern else None
    traffic = pmc_traffic(dom) if n == N_ROWS else None
    b_alg = alg_bytes_expv(n, nnz, m)
    expv_gbps = b_alg / (elapsed / args.steps) / 1e9
    roofline = {
        "bound": "hbm", "kernel": dom,
        "achieved": kern[dom]["alg_GBps"] if dom else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": (kern[dom]["alg_GBps"] / HBM_PEAK_GBS) if dom and kern[dom]["alg_GBps"] else None,
        "traffic": traffic,
        "traffic_source": ("replayed from the committed rocprofv3 PMC pass %s (FETCH_SIZE / WRITE_SIZE in separate runs of this "
                           "command, gfx950 read correction; counters cannot be collected from inside the timed process)"
                           % pmc_traffic_file()) if traffic is not None else None,
        "avg_launch_ms": kern[dom]["avg_ms"] if dom else None,
        "alg_bytes_per_launch": kern[dom]["alg_bytes_per_launch"] if dom else None,
        "expv_alg_GBps": expv_gbps, "expv_frac": expv_gbps / HBM_PEAK_GBS,
        "kernels": kern,
    }
    if pipeline:
        roofline["note"] = ("pipe_step = the single-pass step kernel, one launch per Krylov step; bytes per launch = SURVEY "
                            "§8d A_B + 8n(j+2) averaged over j = 1..m; consecutive launches overlap (two streams), so "
                            "avg_launch_ms = factorisation span / steps; 'serial' = the same kernels one after the other "
                            "(per-launch HIP events)")
        roofline["serial"] = serial

    out = {
        "metric": "expv matvecs/s (Krylov steps/s), n=1e6 5-diagonal sparse fp64, m=30",
        "value": value, "unit": "matvecs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: expv(1.0, A, b), n=%d, offsets (-2..2) diagonals "
                               "(0.3,1.2,-2.0,0.8,-0.1), nnz=%d, m=30, tol=1e-7, full Arnoldi (%s), "
                               "one independent problem per GPU" % (n, nnz, args.ortho),
                   "n": n, "m": m, "nnz": int(nnz), "ortho": args.ortho, "setup_s": t_setup,
                   "entry": "arnoldi!+expv!" if args.split_api else "expv(t,A,b)", "path": path,
                   "outputs": "complete on return" if args.sync_outputs else "stream-ordered",
                   "spinup_calls": spin_calls,
                   "value_cold": cold["value"] if cold else None, "ms_per_step_cold": cold["ms_per_step"] if cold else None},
        "ranks_seen": seen, "devices": ids, "per_rank_ms_per_step": per_rank_ms, "process_group": env.backend,
        "counters": ctx.counters() if ctx is not None else None,
    }
    if args.full:
        out["roofline"] = roofline
    if args.full and rank == 0 and world == 1 and not args.no_secondary and n == N_ROWS and not args.split_api and ctx is not None:
        sec = secondary_block(args, eu, env, op, b, w, n, nnz, m)
        # the driver's record keeps the head of this line: the figures the verdicts ask about are repeated up front, in
        # `config` (the full entries follow in `secondary`)
        sa = sec.get("split_api_sync_outputs", {})
        out["config"]["split_api_sync_outputs"] = {"value": sa.get("value"), "frac": sa.get("frac"), "ms_per_call": sa.get("ms_per_call"),
                                                   "what": "arnoldi!(Ks,A,b) + expv!(w,t,Ks), results complete on return (the Julia shim's path)"}
        summ = {}
        for k_, e_ in sec.items():
            if isinstance(e_, dict) and e_.get("frac") is not None:
                summ[k_] = round(float(e_["frac"]), 3)
        sm = sec.get("small_systems", {})
        for k_, e_ in sm.items():
            if isinstance(e_, dict) and "us_per_krylov_step" in e_:
                summ["small_systems." + k_ + ".us_per_step"] = round(float(e_["us_per_krylov_step"]), 2)
        out["config"]["secondary_fracs"] = summ
        out["config"]["secondary_fracs_minmax"] = {k_: [round(float(v_), 3) for v_ in e_["frac_min_max"]] for k_, e_ in sec.items()
                                                   if isinstance(e_, dict) and "frac_min_max" in e_}
        out["config"]["reordered_setup_s"] = {k_: [round(float(sec[k_]["setup_s"]), 3), round(float(sec[k_]["setup_again_s"]), 3)]
                                    for k_ in ("general_sparse_rcm", "general_sparse_rcm_grid", "general_sparse_mesh") if k_ in sec and "setup_again_s" in sec[k_]}
        out["secondary"] = sec
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and ctx is not None:
        eu.expv(T_FINAL, op, b, m=m, ishermitian=False, ortho=args.ortho, out=w)
        env.sync()
        out["cpu_baseline"] = cpu_baseline_block(A, b_host, w.cpu().numpy(), m, n)
    if env.standin:
        out["standin"] = env.standin
        out["data"] = "stand-in solver on CPU (plumbing test of the launch / sharding / collective code: NOT a measurement)"
    if rank == 0:
        emit(out)
    return out


if __name__ == "__main__":
    main()
