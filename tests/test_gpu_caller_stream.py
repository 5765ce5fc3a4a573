"""A context on a stream of the caller's, and stream-ordered outputs.

include/expv_mi.h promises that `expv_mi_ctx_create(device, stream, ...)` launches on an existing stream of the host's, and that with
`expv_mi_ctx_set_async_outputs` device outputs are "valid for later work on the context's stream".  Every other GPU test runs on a
stream the library created for itself and looks at results after a synchronisation; here ONE torch stream S, created in this file,
carries every case:

1. the same call on `Context(stream=S)` and on a default context: bit for bit the same H, V, m, flags, statistics and results, the
   results at the bar the entry's own test holds against the oracle / the truth, and the counters / path words of the intended form;
2. inputs produced EARLIER on S (delay kernel + copy, no host synchronisation): the library must stay behind them.  The buffer holds a
   valid decoy until the copy lands; tests/test_caller_stream_cpu.py shows that the decoy's answer is >= 1e3 bars away.  A case whose
   producer is not provably still pending right before the call FAILS as vacuous.  One control calls the library on a PRIVATE stream
   through ctypes: it must return the decoy's answer, which proves the method sees a missing edge;
3. outputs consumed LATER on S (`out.clone()` under `torch.cuda.stream(S)`, no ctx.sync(), no device-wide synchronise) with
   async_outputs, compared bit for bit with a complete-on-return context;
4. ownership: S survives the context, two contexts share S, the null stream is refused.

Delays are sized per case: five times the measured wall time of the same call with ready inputs (never below DELAY_FLOOR_MS);
profiles/caller_stream.txt records call time, delay, the pending-producer condition and the outcome of every case."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import scipy.linalg as sl

from oracle import krylov_oracle as ko
from tests import stream_cases as sc
from tests._util import c2_operator, close
from tests.option_forms import OPTION_SETS, context_with
from tests.test_gpu_option_forms import KIOPS_KW, KIOPS_N, KIOPS_STATS, _kiops_inputs, _kiops_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_FLOOR_MS = 30.0
DELAY_FACTOR = 5.0
REPORT = []
N, T_STEP = sc.N, sc.T_STEP


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def S(torch):
    """THE caller's stream of this file (a process has four hardware queues, and the library adds a second stream of its own)"""
    return torch.cuda.Stream()


@pytest.fixture(scope="module")
def delay(torch):
    d = sc.Delay(torch)
    d.calibrate()
    return d


@pytest.fixture(scope="module")
def ctxs(eu, S):
    """(context on S, context on a private stream) per (option set, async outputs on S); the private one always completes on return"""
    made = {}

    def get(oset="default", async_outputs=False):
        opts = OPTION_SETS[oset] if isinstance(oset, str) else dict(oset)
        key = (tuple(sorted(opts.items())), async_outputs)
        if key not in made:
            made[key] = (context_with(eu, opts, stream=S, async_outputs=async_outputs), context_with(eu, opts))
        return made[key]
    return get


@pytest.fixture(scope="module", autouse=True)
def _write_report(request):
    """profiles/caller_stream.txt, rewritten only by a run of the WHOLE module (no -k, no node ids): a partial run leaves the file alone"""
    yield
    cfg = request.config
    if not REPORT or cfg.option.keyword or any("::" in str(a) for a in cfg.args):
        return
    try:
        with open(os.path.join(ROOT, "profiles", "caller_stream.txt"), "w") as f:
            f.write("# written by tests/test_gpu_caller_stream.py (-m gpu): one torch stream S carries every case\n")
            f.write("# same_bits: Context(stream=S) vs a default context, every product bit for bit; late_input: delay + copy of the real input queued on S before\n")
            f.write("# the call (call_ms: the same call with ready inputs; delay_ms >= %g x that, floor %g ms; pending: the producer's event had not\n" % (DELAY_FACTOR, DELAY_FLOOR_MS))
            f.write("# completed right before the call); late_output: out.clone() queued on S after the call, no synchronisation in between\n")
            f.write("# %-12s %-58s %9s %9s %-8s %s\n" % ("kind", "case", "call_ms", "delay_ms", "pending", "outcome"))
            for kind, case, call_ms, delay_ms, pending, outcome in REPORT:
                f.write("%-14s %-58s %9s %9s %-8s %s\n" % (kind, case, "-" if call_ms is None else "%.3f" % call_ms,
                                                        "-" if delay_ms is None else "%.1f" % delay_ms, "-" if pending is None else str(pending), outcome))
    except OSError:
        pass


# ------------------------------------------------------------------------------------------- helpers
def _differences(a, b):
    """names of the products that are not bit-for-bit equal"""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        else:
            same = x == y
        if not same:
            bad.append(k)
    return bad


def _same_on_both(ctxs, oset, run, label):
    """run(ctx) -> {name: product} on the context on S and on a private one: (a) of the module docstring.  Returns the products of S.
    (Were an entry not reproducible run to run, the message says so: the private context is then run a second time.)"""
    cS, cP = ctxs(oset)
    rS, rP = run(cS), run(cP)
    bad = _differences(rS, rP)
    note = ""
    if bad:
        again = _differences(rP, run(cP))
        note = "; two runs on the private context differ in %r" % again if again else "; two runs on the private context agree bit for bit"
    REPORT.append(("same_bits", label, None, None, None, "bit-identical" if not bad else "DIFFERS in %r%s" % (bad, note)))
    assert not bad, "%s: caller's stream vs private stream differ in %r%s" % (label, bad, note)
    return rS


def _counter_delta(ctx, fn):
    c0 = ctx.counters()
    out = fn()
    c1 = ctx.counters()
    return out, {k: c1[k] - c0[k] for k in c1}


def _assert_form(d, words, label, nfact=1):
    want = {"factorisations": nfact, "pipeline": nfact if "pipeline" in words else 0, "overlapped": nfact if "overlapped" in words else 0,
            "redo_serial": 0, "redo_wave_off": 0}
    got = {k: d[k] for k in want}
    assert got == want, "%s: counters %r, expected %r" % (label, got, want)


def _expv(eu, ctx, op, b, words, label, **kw):
    """one whole-call expv with the path words and the counters of its form asserted"""
    w, d = _counter_delta(ctx, lambda: eu.expv(T_STEP, op, b, **kw))
    st = dict(eu.expv.last_stats)
    path = frozenset(st["path"])
    assert words <= path and not (path - words - {"fa2_pipelined"}), "%s: ran on %s, expected %s" % (label, sorted(path), sorted(words))
    _assert_form(d, words, label)
    st["counters"] = d
    return w, st


def _colmajor(torch, M):
    """a column-major device tensor holding M"""
    M = np.asarray(M)
    if M.ndim == 1:
        return torch.as_tensor(np.ascontiguousarray(M), device="cuda")
    return torch.as_tensor(np.ascontiguousarray(M.T), device="cuda").t()


# ------------------------------------------------------------------------------------------- 1. the same arithmetic on a caller's stream
PIPE, PIPE_SERIAL, TWO_KERNEL, MODULAR = frozenset({"pipeline", "overlapped"}), frozenset({"pipeline"}), frozenset({"two_kernel"}), frozenset({"modular"})
EXPV_ENTRIES = {
    # name: (operator, element type, option set, path words)
    "banded_float64_overlapped": ("banded", np.float64, "default", PIPE),
    "banded_float64_overlap_off": ("banded", np.float64, "pipeline_serial", PIPE_SERIAL),
    # H by copy on the context's stream instead of through the mailbox: the copy is ordered behind the helper stream's last step (m
    # even) by the join event alone.  Also at 70 001 rows, where that step is long enough for an early copy to miss its column.
    "banded_float64_overlapped_h_by_copy": ("banded", np.float64, "mailbox0", PIPE),
    "banded_float64_overlapped_h_by_copy_70001": ("banded", np.float64, "mailbox0", PIPE, 70_001),
    "general_sparse_two_kernel": ("random_rows", np.float64, "fa2_pipelined1_reorder0_pipeline0", TWO_KERNEL),
    "dense_operator": ("dense", np.float64, "default", MODULAR),
    "banded_complex128": ("banded", np.complex128, "default", PIPE),
    "banded_float32": ("banded", np.float32, "default", PIPE),
}


def _operator(kind, T, n=N):
    if kind == "banded":
        return sc.banded(n, T)
    if kind == "random_rows":
        return sc.random_rows(n, T)
    return sc.dense_operator(130, T)


@pytest.mark.parametrize("entry", list(EXPV_ENTRIES))
def test_expv_on_a_callers_stream(eu, ctxs, entry):
    """expv on each operator class: overlapped single-pass step (second stream, fork and join events), the same with the overlap off,
    two-kernel step, modular launches (dense), ComplexF64 and Float32 -- same bits as on a private stream, the oracle's answer at TOL
    (2e-5 for Float32), and the path words + counters of the form."""
    kind, T, oset, words = EXPV_ENTRIES[entry][:4]
    A = _operator(kind, T, *EXPV_ENTRIES[entry][4:])
    n = A.shape[0]
    b = sc.vector(n, T, 0)
    m = sc.krylov_m(T)

    def run(ctx):
        op = eu.MIOperator(A, ctx)
        w, st = _expv(eu, ctx, op, b, words, entry, m=m, ishermitian=False)
        # (the rule of test_gpu_option_forms._counted: the mailbox serves the overlapped step and the whole-call two-kernel step)
        by_mailbox = oset != "mailbox0" and ("overlapped" in words or "two_kernel" in words)
        assert st["counters"]["h_by_copy"] == (0 if by_mailbox else 1), (entry, st["counters"])
        return {"w": np.asarray(w), "m": st["m"], "wasbreakdown": st["wasbreakdown"], "matvecs": st["matvecs"], "beta": st["beta"],
                "path": frozenset(st["path"]), "fa2_pipelined": st["fa2_pipelined"]}
    r = _same_on_both(ctxs, oset, run, "expv " + entry)
    T64 = sc.wide(T)
    want = ko.expv(T_STEP, A.astype(T64), b.astype(T64), m=m, ishermitian=False)
    close(r["w"].astype(T64), want, sc.TOL32_W if np.dtype(T) == np.float32 else sc.TOL, "caller's stream, expv %s vs oracle" % entry)


def test_matrix_free_callback_is_handed_the_callers_stream(eu, torch, S, ctxs):
    """A matrix-free operator whose callback launches the library's own stream-ordered dense product (expv_mi_gemv_block, as
    dist.py does): the callback of the context on S is handed S itself, every time; same bits as on a private stream, the oracle's
    answer at the matrix-free bar (1e-10, test_matrix_free_operator_on_the_two_kernel_step_odd_sizes)."""
    n, m = 130, 30
    rng = np.random.default_rng([5055, n])
    A = rng.standard_normal((n, n)) / np.sqrt(n) - 0.5 * np.eye(n)
    b = rng.standard_normal(n)
    Ad = _colmajor(torch, A)
    lib = eu.api.L.load()
    handed = {}

    def run(ctx):
        seen = handed.setdefault(id(ctx), [])

        def cb(user, xp, yp, stream):
            seen.append(int(stream or 0))
            return lib.expv_mi_gemv_block(ctx._h, eu.api.L.F64, n, n, Ad.data_ptr(), n, xp, yp, None, 1)
        fn = eu.api.L.MATVEC_FN(cb)
        op = eu.MIOperator(None, ctx, matvec_c=(fn, None), shape=(n, n), dtype=np.float64, ishermitian=False)
        w, d = _counter_delta(ctx, lambda: eu.expv(0.7, op, b, m=m, ishermitian=False))
        st = dict(eu.expv.last_stats)
        assert d["factorisations"] == 1 and d["pipeline"] == 0 and set(st["path"]) & {"two_kernel", "modular"}, (d, st)
        return {"w": np.asarray(w), "m": st["m"], "path": frozenset(st["path"]), "matvecs": st["matvecs"], "applications": len(seen)}
    r = _same_on_both(ctxs, "default", run, "matrix-free callback")
    cS, cP = ctxs("default")
    assert handed[id(cS)] and set(handed[id(cS)]) == {int(S.cuda_stream)}, (set(handed[id(cS)]), S.cuda_stream)
    assert S.cuda_stream not in set(handed[id(cP)]) and 0 not in set(handed[id(cP)])
    close(r["w"], ko.expv(0.7, A, b, m=m, ishermitian=False), sc.TOL_MATFREE, "caller's stream, matrix-free expv vs oracle")


def test_split_api_on_a_callers_stream(eu, ctxs):
    """arnoldi!(defer_tail) -> Ks.H / getV -> expv!: the deferred closing pass is collected behind the caller's stream too."""
    A, b, m = sc.banded(N, np.float64), sc.vector(N, np.float64, 0), 20

    def run(ctx):
        op = eu.MIOperator(A, ctx)
        Ks = eu.KrylovSubspace(np.float64, np.float64, N, m + 2, 0, ctx)
        _, d = _counter_delta(ctx, lambda: eu.arnoldi_(Ks, op, b, m=m, ishermitian=False, defer_tail=True))
        _assert_form(d, PIPE, "arnoldi!(defer_tail)")
        H = np.asarray(Ks.getH()).copy()
        V = np.asarray(Ks.getV()).copy()
        w = np.asarray(eu.expv_(np.empty(N), 0.4, Ks)).copy()
        return {"H": H, "V": V, "w": w, "m": Ks.m, "wasbreakdown": Ks.wasbreakdown, "beta": Ks.beta, "Hfull": np.asarray(Ks.H).copy()}
    r = _same_on_both(ctxs, "default", run, "arnoldi!(defer_tail), H, getV, expv!")
    Ko = ko.arnoldi(A, b, m=m, ishermitian=False)
    assert r["m"] == Ko.m and bool(r["wasbreakdown"]) == bool(Ko.wasbreakdown)
    close(r["H"], Ko.getH(), sc.TOL, "caller's stream, arnoldi! H", mat=True)
    close(r["V"], Ko.getV(), sc.TOL, "caller's stream, arnoldi! V (max abs)", absolute=True)
    close(r["w"], ko.expv_(np.empty(N), 0.4, Ko), sc.TOL, "caller's stream, expv! of the subspace")


def test_lanczos_and_phiv_on_a_callers_stream(eu, ctxs):
    A, b, m, k = sc.hermitian_part(sc.banded(N, np.float64)), sc.vector(N, np.float64, 0), 20, 2

    def run(ctx):
        op = eu.MIOperator(A, ctx)
        Ks = eu.KrylovSubspace(np.float64, np.float64, N, m, 0, ctx)
        _, d = _counter_delta(ctx, lambda: eu.lanczos_(Ks, op, b, m=m))
        _assert_form(d, PIPE, "lanczos!")
        W, est = eu.phiv_(np.empty((N, k + 1), order="F"), 0.5, Ks, k, correct=True, errest=True)
        return {"H": np.asarray(Ks.getH()).copy(), "V": np.asarray(Ks.getV()).copy(), "W": np.asarray(W).copy(), "errest": float(est), "m": Ks.m,
                "wasbreakdown": Ks.wasbreakdown}
    r = _same_on_both(ctxs, "default", run, "lanczos!, phiv!(correct, errest)")
    Ko = ko.arnoldi(A, b, m=m, ishermitian=True)
    Wo, esto = ko.phiv_(np.empty((N, k + 1), order="F"), 0.5, Ko, k, correct=True, errest=True)
    assert r["m"] == Ko.m
    close(r["H"], np.real(Ko.getH()), sc.TOL, "caller's stream, lanczos! H", mat=True)
    close(r["V"], Ko.getV(), sc.TOL, "caller's stream, lanczos! V (max abs)", absolute=True)
    close(r["W"], Wo, sc.TOL, "caller's stream, phiv!(k=2, correct)")
    assert np.isfinite(r["errest"])
    if esto > 1e-10 * float(np.linalg.norm(Wo)):      # (the rule of test_option_form_matches_oracle: where the estimate is more than rounding noise)
        close(r["errest"], esto, 1e-6, "caller's stream, phiv! error estimate")


def test_phiv_timestep_on_a_callers_stream(eu, ctxs):
    """the adaptive time stepper (operator, B, ts and options of test_adaptive_timestep_after_a_failed_call_on_the_same_context)"""
    n = KIOPS_N
    A = c2_operator(n)
    B = np.asfortranarray(np.random.default_rng(22).standard_normal((n, 3)))
    ts = np.array([0.4, 1.0])
    kw = dict(adaptive=True, tol=1e-8, m=20)

    def run(ctx):
        op = eu.MIOperator(A, ctx)
        st = {}
        U, d = _counter_delta(ctx, lambda: eu.phiv_timestep(ts.copy(), op, B, stats=st, **kw))
        assert d["factorisations"] >= 1 and d["pipeline"] == d["factorisations"] and d["overlapped"] >= 1 and d["redo_serial"] == d["redo_wave_off"] == 0, d
        return {"U": np.asarray(U).copy(), "counters": tuple(sorted(d.items())), **st}
    r = _same_on_both(ctxs, "default", run, "phiv_timestep (adaptive)")
    so = {}
    Uo = ko.phiv_timestep(ts.copy(), A, B, stats=so, **kw)
    assert (r["num_timesteps"], r["matvecs"], r["m"]) == (so["num_timesteps"], so["matvecs"], so["m"]), (r, so)
    close(r["U"], Uo, sc.TOL, "caller's stream, phiv_timestep (adaptive) vs oracle")


def test_kiops_with_a_rejected_substep_on_a_callers_stream(eu, ctxs):
    """operator, u, step and options of test_kiops_skip_redo_both_ways (every run contains a rejection: asserted)"""
    A, u = _kiops_inputs()[False]
    wo, so = _kiops_oracle(False, "iop2_tol1e-10")
    assert so[1] >= 1 and tuple(so) == KIOPS_STATS[(False, "iop2_tol1e-10")], so

    def run(ctx):
        op = eu.MIOperator(A, ctx)
        (w, st), d = _counter_delta(ctx, lambda: eu.kiops(2.0, op, u, ishermitian=False, **KIOPS_KW["iop2_tol1e-10"]))
        assert d["factorisations"] >= 2 and d["overlapped"] == d["pipeline"] == d["factorisations"] and d["redo_serial"] == d["redo_wave_off"] == 0, d
        return {"w": np.asarray(w).copy(), "stats": tuple(st), "counters": tuple(sorted(d.items()))}
    r = _same_on_both(ctxs, "default", run, "kiops with a rejected sub-step")
    assert r["stats"] == tuple(so) and r["stats"][1] >= 1, (r["stats"], so)
    close(r["w"], wo, sc.TOL, "caller's stream, kiops vs oracle")


def test_expv_batch_on_a_callers_stream(eu, ctxs):
    n, nprob, m = N, 5, 16
    rng = np.random.default_rng(n + 16)
    A0 = c2_operator(n).tocsr()
    A0.sort_indices()
    vals = np.stack([A0.data * s for s in (1 + 0.1 * rng.random(nprob))])
    B = np.asfortranarray(rng.standard_normal((n, nprob)))

    def run(ctx):
        W, mu = eu.expv_batch(0.8, A0, vals, B, m=m, ctx=ctx, return_m=True)
        return {"W": np.asarray(W).copy(), "m": np.asarray(mu).copy()}
    r = _same_on_both(ctxs, "default", run, "expv_batch")
    assert all(int(x) == m for x in r["m"])
    for p in range(nprob):
        Ap = A0.copy()
        Ap.data = vals[p].copy()
        close(r["W"][:, p], ko.expv(0.8, Ap, B[:, p], m=m, ishermitian=False), sc.TOL, "caller's stream, expv_batch problem %d vs oracle" % p)


def _dense_inputs(n):
    from tests import dense_cases as dc
    return dc.skew_case("float64", 130, 6, 5.0)["A"] if n == 130 else np.asfortranarray(np.random.default_rng(1096).standard_normal((96, 96)))


def _strip_time(info):
    return {k: v for k, v in info.items() if "microseconds" not in k}


@pytest.mark.parametrize("kind", ["device_array", "torch"])
@pytest.mark.parametrize("n", [96, 130])
def test_dense_entries_on_a_callers_stream(eu, torch, ctxs, n, kind):
    """exponential!, exponential!(balance), phi! and mul! on DeviceArray / torch operands (the matrices of
    test_back_to_back_stream_ordered_calls_share_the_workspace): same bits and the same method (order, squarings, exchanges, degree,
    products) as on a private stream, the truths at 1e-11; the product is exact on small integers."""
    A = _dense_inputs(n)
    k = 2
    Aphi, phi_truth = sc.pc.case("float64", n, 5.0, "randn") if n in sc.pc.PARITY_SIZES else (sc.pc.matrix("float64", n, 5.0, "randn"), None)
    phi_truth = phi_truth[: k + 1] if phi_truth is not None else sc.pc.truth(Aphi, k)
    Ai, Bi = np.asfortranarray(np.random.default_rng(n).integers(-3, 4, (n, 70)).astype(np.float64)), \
        np.asfortranarray(np.random.default_rng(n + 1).integers(-3, 4, (70, n + 3)).astype(np.float64))

    def put(M, ctx):
        return eu.DeviceArray.from_host(M, ctx) if kind == "device_array" else _colmajor(torch, M)

    def get(x):
        return x.to_host() if kind == "device_array" else x.cpu().numpy()

    def run(ctx):
        E, i1 = eu.exponential_(put(A, ctx), ctx=ctx, return_info=True)
        Eb, i2 = eu.exponential_(put(A, ctx), balance=True, ctx=ctx, return_info=True)
        Ad = put(np.array(Aphi), ctx)
        out = [put(np.zeros((n, n), order="F"), ctx) for _ in range(k + 1)]
        _, i3 = eu.phi_(out, Ad, k, ctx=ctx, return_info=True)
        Cm = eu.mul_(put(np.ones((n, n + 3), order="F"), ctx), put(Ai, ctx), put(Bi, ctx), alpha=2, beta=-1, ctx=ctx)
        if kind == "device_array":
            ctx.sync()          # (mul! on DeviceArrays is stream-ordered: to_host reads on the same context, this is belt and braces)
        return {"exp": get(E), "exp_info": _strip_time(i1), "exp_balanced": get(Eb), "exp_balanced_info": _strip_time(i2),
                "phi": np.stack([get(o) for o in out]), "phi_info": _strip_time(i3), "A_after_phi": get(Ad), "mul": get(Cm)}
    r = _same_on_both(ctxs, "default", run, "dense entries n=%d %s" % (n, kind))
    truth = sl.expm(A.astype(np.complex128))
    close(r["exp"], truth, sc.TOL_DENSE["float64"], "caller's stream, exponential! n=%d %s" % (n, kind))
    close(r["exp_balanced"], truth, sc.TOL_DENSE["float64"], "caller's stream, exponential!(balance) n=%d %s" % (n, kind))
    for j, ref in enumerate(phi_truth):
        close(r["phi"][j], ref, sc.TOL_DENSE["float64"], "caller's stream, phi! n=%d %s: phi_%d" % (n, kind, j))
    assert np.array_equal(r["A_after_phi"], Aphi) and np.array_equal(r["mul"], 2 * (Ai @ Bi) - 1)


# ------------------------------------------------------------------------------------------- 2. inputs produced earlier on the caller's stream
def _produce_late(torch, S, delay, buf, real, ms):
    """on S: a delay of `ms`, then the real input into `buf`; the event behind the copy"""
    ev = torch.cuda.Event()
    with torch.cuda.stream(S):
        delay.enqueue(ms)
        buf.copy_(real, non_blocking=True)
        ev.record(S)
    return ev


class LateEntry:
    """one entry of section 2: prep(ctx) -> state kept across calls, fresh(x) -> (buffer the producer writes, what the call is handed),
    call(ctx, state, handle) -> the answer as a numpy array"""
    case = None

    def __init__(self, eu, torch):
        self.eu, self.torch, self.c = eu, torch, sc.late_cases()[self.case]

    def prep(self, ctx):
        return None

    def fresh(self, x):
        t = _colmajor(self.torch, x)
        return t, t


class ExpvDeviceB(LateEntry):
    case = "expv_device_b"

    def prep(self, ctx):
        return self.eu.MIOperator(self.c.A, ctx)

    def call(self, ctx, op, b):
        w, st = _expv(self.eu, ctx, op, b, PIPE, self.case, m=self.c.m, ishermitian=False)
        return w.cpu().numpy()


class ArnoldiDeviceB(ExpvDeviceB):
    case = "arnoldi_device_b"

    def call(self, ctx, op, b):
        Ks = self.eu.KrylovSubspace(np.float64, np.float64, N, self.c.m, 0, ctx)
        _, d = _counter_delta(ctx, lambda: self.eu.arnoldi_(Ks, op, b, m=self.c.m, ishermitian=False))
        _assert_form(d, PIPE, self.case)
        assert Ks.m == self.c.m and not Ks.wasbreakdown
        return np.asarray(Ks.getV())[:, : self.c.m + 1]


class CsrValues(LateEntry):
    """MIOperator from device CSR arrays (expv_mi_op_create_csr_loc) whose values are still being produced"""
    case = "csr_values"

    def fresh(self, x):
        torch, A = self.torch, self.c.A
        vals = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
        At = torch.sparse_csr_tensor(torch.as_tensor(A.indptr.astype(np.int32), device="cuda"), torch.as_tensor(A.indices.astype(np.int32), device="cuda"),
                                     vals, size=A.shape)
        assert At.values().data_ptr() == vals.data_ptr()      # (the tensor aliases the buffer the producer writes)
        return vals, At

    def call(self, ctx, state, At):
        op = self.eu.MIOperator(At, ctx)
        assert op.ingest_info["from_device"] and op.ingest_info["value_bytes_to_host"] == 0
        w, _ = _expv(self.eu, ctx, op, self.c.b, PIPE, self.case, m=self.c.m, ishermitian=False)
        return np.asarray(w)


class UpdateValues(LateEntry):
    case = "update_values"

    def prep(self, ctx):
        A = self.c.A.copy()
        A.data = np.asarray(self.c.x[0]).copy()
        return self.eu.MIOperator(A, ctx)

    def call(self, ctx, op, vals):
        op.update_values(vals)
        w, _ = _expv(self.eu, ctx, op, self.c.b, PIPE, self.case, m=self.c.m, ishermitian=False)
        return np.asarray(w)


class DenseOperator(LateEntry):
    """the case of the comment in api.py (_Arg): a dense device operator read while it is still being written"""
    case = "dense_operator"

    def call(self, ctx, state, Ad):
        op = self.eu.MIOperator(Ad, ctx)
        w, _ = _expv(self.eu, ctx, op, self.c.b, MODULAR, self.case, m=self.c.m, ishermitian=False)
        return np.asarray(w)


class Exponential(LateEntry):
    case = "exponential"

    def call(self, ctx, state, Ad):
        return self.eu.exponential_(Ad, ctx=ctx).cpu().numpy()


class Phi(LateEntry):
    case = "phi"

    def call(self, ctx, state, Ad):
        return np.stack([p.cpu().numpy() for p in self.eu.phi(Ad, self.c.k, ctx=ctx)])


class Mul(LateEntry):
    case = "mul"

    def call(self, ctx, state, Bd):
        Cm = _colmajor(self.torch, np.full((self.c.A.shape[0], Bd.shape[1]), np.nan))
        return self.eu.mul_(Cm, _colmajor(self.torch, self.c.A), Bd, ctx=ctx).cpu().numpy()


class GemvBlock(LateEntry):
    """expv_mi_gemv_block through ctypes: "stream-ordered: nothing is synchronised" """
    case = "gemv_block"

    def call(self, ctx, state, xd):
        nr, nc = self.c.A.shape
        Ad = _colmajor(self.torch, self.c.A)
        yd = self.torch.full((nr,), float("nan"), dtype=self.torch.float64, device="cuda")
        self.torch.cuda.current_stream().synchronize()      # (Ad and yd are ready; the caller's stream S is not touched)
        rc = self.eu.api.L.load().expv_mi_gemv_block(ctx._h, self.eu.api.L.F64, nr, nc, Ad.data_ptr(), nr, xd.data_ptr(), yd.data_ptr(), None, 1)
        assert rc == 0
        ctx.sync()
        return yd.cpu().numpy()


LATE_ENTRIES = [ExpvDeviceB, ArnoldiDeviceB, CsrValues, UpdateValues, DenseOperator, Exponential, Phi, Mul, GemvBlock]


def _check(case, got, which, what):
    e = sc.err(got, case.want(which), case.mode)
    print("[parity] %-90s err %.3e  (bar %.1e)" % (what, e, case.bar))
    return e


@pytest.mark.parametrize("entry", LATE_ENTRIES, ids=[e.case for e in LATE_ENTRIES])
def test_input_produced_earlier_on_the_callers_stream(eu, torch, S, delay, ctxs, entry):
    """Module docstring, 2.  The call with ready inputs first (on the private context: the wall time that sizes the delay, and the decoy's
    answer, which shows that a stale read WOULD be seen; on the context on S: its workspaces exist), then the late input."""
    E = entry(eu, torch)
    case = E.c
    cS, cP = ctxs("default")
    sP, sS = E.prep(cP), E.prep(cS)
    assert _check(case, E.call(cP, sP, E.fresh(case.x[0])[1]), 0, "%s: ready decoy on the private context" % case.name) <= case.bar
    h = E.fresh(case.x[0])[1]
    torch.cuda.synchronize()
    _, call_ms = sc.timed(lambda: E.call(cP, sP, h))
    assert _check(case, E.call(cS, sS, E.fresh(case.x[0])[1]), 0, "%s: ready decoy on the caller's stream" % case.name) <= case.bar
    buf, handle = E.fresh(case.x[0])
    real = E.fresh(case.x[1])[0]
    torch.cuda.synchronize()
    wait_ms = max(DELAY_FACTOR * call_ms, DELAY_FLOOR_MS)
    ev = _produce_late(torch, S, delay, buf, real, wait_ms)
    pending = not ev.query()                     # immediately before the library call
    got = E.call(cS, sS, handle)
    S.synchronize()
    e1, e0 = sc.err(got, case.want(1), case.mode), sc.err(got, case.want(0), case.mode)
    print("[parity] %-90s err %.3e  (bar %.1e; distance to the decoy's answer %.3e)" % (case.name + ": late input on the caller's stream", e1, case.bar, e0))
    REPORT.append(("late_input", case.name, call_ms, wait_ms, pending, "err %.3e (bar %.1e), decoy's answer %.3e away" % (e1, case.bar, e0)))
    assert pending, "%s is vacuous: the producer had completed before the call (call %.3f ms, delay %.1f ms)" % (case.name, call_ms, wait_ms)
    assert e1 <= case.bar, "%s: the library did not stay behind the producer on its stream: err %.3e > bar %.1e (decoy's answer: %.3e away)" % (
        case.name, e1, case.bar, e0)


def test_control_a_private_stream_reads_the_decoy(eu, torch, S, delay, ctxs):
    """The control: the expv case through ctypes with raw pointers on a context with a PRIVATE stream, which has no edge to S -- it must
    return the DECOY's answer while the producer is still pending (valid memory only: the buffer holds the decoy until the copy
    lands, which is after the call has returned).  The method can see a missing edge.
    It is the control of the expv entry alone.  The entries that create or refill an operator (device CSR, update_values, a dense
    operator) synchronise the stream inside the call to bring properties home: their answers prove the contract held, not whether
    the order came from the stream or from such a synchronisation."""
    case = sc.late_cases()["expv_device_b"]
    L = eu.api.L
    lib = L.load()
    _, cP = ctxs("default")
    op = eu.MIOperator(case.A, cP)
    buf, real = _colmajor(torch, case.x[0]), _colmajor(torch, case.x[1])
    w = torch.zeros(N, dtype=torch.float64, device="cuda")
    o = eu.api._opts(case.m, 1e-7, 0, 0, False, "auto")
    st = L.ExpvStats()

    def call():
        assert lib.expv_mi_expv(cP._h, op._h, T_STEP, 0.0, buf.data_ptr(), L.DEVICE, w.data_ptr(), L.DEVICE, L.F64, C.byref(o), C.byref(st)) == 0
    call()
    torch.cuda.synchronize()
    _, call_ms = sc.timed(call)
    wait_ms = max(DELAY_FACTOR * call_ms, DELAY_FLOOR_MS)
    ev = _produce_late(torch, S, delay, buf, real, wait_ms)
    before = not ev.query()
    call()                                        # complete on return (the private context's outputs are not stream-ordered)
    after = not ev.query()
    got = w.cpu().numpy()
    S.synchronize()
    e0, e1 = sc.err(got, case.want(0)), sc.err(got, case.want(1))
    REPORT.append(("control", "expv through ctypes on a private stream", call_ms, wait_ms, before and after, "decoy's answer: err %.3e (bar %.1e); real answer %.3e away" % (e0, case.bar, e1)))
    assert before and after, "the control is vacuous: the producer completed during the call (call %.3f ms, delay %.1f ms)" % (call_ms, wait_ms)
    assert e0 <= case.bar and e1 >= 1e3 * case.bar, (e0, e1)
    assert np.array_equal(buf.cpu().numpy(), case.x[1])      # (the producer did run afterwards)


def test_helper_stream_stays_behind_a_busy_callers_stream(eu, torch, S, delay, ctxs):
    """The fork edge of the overlapped step: the helper stream's kernels (the even steps) must not start before what the context's
    stream has queued in front of them.  The step flags make an early start harmless for the NUMBERS -- such a kernel polls until
    its predecessor is done -- but only within spin_limit polls; beyond them it gives up and the host redoes the factorisation one
    launch after the other (counter redo_serial).  So: a context on S whose kernels give up after 20 000 polls (512 cycles of sleep +
    one load each: 5 .. 40 ms; the default of 400 000 is for a device shared with other work), the late-input expv behind a delay of at
    least 150 ms.  With the edge in place no kernel of the helper stream runs during the delay and nothing is redone."""
    E = ExpvDeviceB(eu, torch)
    case = E.c
    cS, cP = ctxs({"spin_limit": 20_000})
    sP, sS = E.prep(cP), E.prep(cS)
    h = E.fresh(case.x[0])[1]
    E.call(cP, sP, h)
    torch.cuda.synchronize()
    _, call_ms = sc.timed(lambda: E.call(cP, sP, h))
    assert _check(case, E.call(cS, sS, E.fresh(case.x[0])[1]), 0, "short spin limit: ready decoy on the caller's stream") <= case.bar
    buf, handle = E.fresh(case.x[0])
    real = E.fresh(case.x[1])[0]
    torch.cuda.synchronize()
    wait_ms = max(DELAY_FACTOR * call_ms, 150.0)
    ev = _produce_late(torch, S, delay, buf, real, wait_ms)
    pending = not ev.query()
    c0 = cS.counters()
    try:
        got = E.call(cS, sS, handle)              # (asserts the overlapped form and redo_serial == 0 itself)
    finally:
        S.synchronize()
        c1 = cS.counters()
        REPORT.append(("late_input", "expv_device_b, spin_limit 20000", call_ms, wait_ms, pending,
                       "redo_serial %d, overlapped %d" % (c1["redo_serial"] - c0["redo_serial"], c1["overlapped"] - c0["overlapped"])))
    assert pending, "vacuous: the producer had completed before the call (call %.3f ms, delay %.1f ms)" % (call_ms, wait_ms)
    assert _check(case, got, 1, "short spin limit: late input on the caller's stream") <= case.bar


def test_complete_on_return_waits_for_a_busy_callers_stream(eu, torch, S, delay, ctxs):
    """expv!(w, t, Ks) with a device w on a context on S whose outputs are complete on return, while S is still busy with the caller's
    earlier work: the host has nothing to wait for before the combine is queued (H is on the host already), so the ONLY thing that
    makes w complete on return is the synchronisation behind the combine.  Right after the call: the caller's earlier work is over
    (the call waited for the stream), and a torch .cpu() on the default stream -- no edge to S -- reads the finished result."""
    cS, cP = ctxs("default")
    A, b, m = sc.banded(N, np.float64), sc.vector(N, np.float64, 0), 20
    res = {}
    for ctx in (cP, cS):
        op = eu.MIOperator(A, ctx)
        Ks = eu.KrylovSubspace(np.float64, np.float64, N, m, 0, ctx)
        eu.arnoldi_(Ks, op, b, m=m, ishermitian=False)
        Ks.getH()                                   # (collects the deferred closing pass: nothing of the factorisation is pending)
        w = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        eu.expv_(w, 0.4, Ks)                        # warm: the coefficient buffers exist
        w.fill_(float("nan"))
        torch.cuda.synchronize()
        if ctx is cS:
            _, call_ms = sc.timed(lambda: eu.expv_(w, 0.4, Ks))
            w.fill_(float("nan"))
            torch.cuda.synchronize()
            wait_ms = max(DELAY_FACTOR * call_ms, DELAY_FLOOR_MS)
            ev = torch.cuda.Event()
            with torch.cuda.stream(S):
                delay.enqueue(wait_ms)
                ev.record(S)
            pending = not ev.query()
            eu.expv_(w, 0.4, Ks)
            waited = ev.query()
            res[ctx] = w.cpu().numpy()                # on the default stream, at once
            S.synchronize()
        else:
            eu.expv_(w, 0.4, Ks)
            res[ctx] = w.cpu().numpy()
    same = np.array_equal(res[cS], res[cP])
    REPORT.append(("late_output", "expv! complete on return on a busy S", call_ms, wait_ms, pending,
                   "%s; the call %s for the stream" % ("bit-identical to the private stream" if same else "DIFFERS (NaN left: %d)" % int(np.isnan(res[cS]).sum()),
                                                       "waited" if waited else "did NOT wait")))
    assert pending, "vacuous: the delay had completed before the call (call %.3f ms, delay %.1f ms)" % (call_ms, wait_ms)
    assert waited and same
    close(res[cS], ko.expv_(np.empty(N), 0.4, ko.arnoldi(A, b, m=m, ishermitian=False)), sc.TOL, "expv! on a busy caller's stream vs oracle")


# ------------------------------------------------------------------------------------------- 3. outputs consumed later on the caller's stream
def _consume_on(torch, S, *outs):
    """the consumer: clones queued on S; then S alone is synchronised"""
    with torch.cuda.stream(S):
        clones = [o.clone() for o in outs]
    S.synchronize()
    return [c.cpu().numpy() for c in clones]


def _late_output(label, got, want):
    same = all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    REPORT.append(("late_output", label, None, None, None, "bit-identical to the complete-on-return context" if same else "DIFFERS"))
    assert same, "%s: consumed on the caller's stream differs from the complete-on-return context" % label


@pytest.mark.parametrize("entry", ["overlapped", "reordered"])
def test_expv_output_consumed_on_the_callers_stream(eu, torch, S, ctxs, entry):
    """async_outputs on S: w of expv is read by work queued on S after the call, with no synchronisation in between -- the overlapped
    single-pass step, and a reordered operator (result un-permuted on the way out)."""
    oset, A, words = ("default", sc.banded(N, np.float64), PIPE) if entry == "overlapped" else ("reorder2", sc.random_rows(N, np.float64), None)
    cA, cP = ctxs(oset, async_outputs=True)
    b = sc.vector(N, np.float64, 0)
    opP, opA = eu.MIOperator(A, cP), eu.MIOperator(A, cA)
    if entry == "reordered":
        assert opA.reorder_info["reordered"] and opP.reorder_info["reordered"]
    want = np.asarray(eu.expv(T_STEP, opP, b, m=20, ishermitian=False))
    path = frozenset(eu.expv.last_stats["path"])
    close(want, ko.expv(T_STEP, A, b, m=20, ishermitian=False), sc.TOL, "complete-on-return context, expv %s vs oracle" % entry)
    bd, out = torch.as_tensor(b, device="cuda"), torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert words is None or path == words, (path, words)
    _expv(eu, cA, opA, bd, path, "late output, expv " + entry, m=20, ishermitian=False, out=out)      # (same path words as the private context, its counters, nothing redone)
    got, = _consume_on(torch, S, out)
    _late_output("expv " + entry, [got], [want])


@pytest.mark.parametrize("entry", ["banded", "reordered"])
def test_matrix_valued_phiv_output_consumed_on_the_callers_stream(eu, torch, S, ctxs, entry):
    """phiv! with a device matrix as output; on a reordered operator its columns are un-permuted through a pooled temporary that goes
    back to the context's spares when the call returns"""
    oset, A = ("default", sc.banded(N, np.float64)) if entry == "banded" else ("reorder2", sc.random_rows(N, np.float64))
    cA, cP = ctxs(oset, async_outputs=True)
    b, m, k = sc.vector(N, np.float64, 0), 20, 2
    res = []
    for ctx in (cP, cA):
        op = eu.MIOperator(A, ctx)
        assert entry == "banded" or op.reorder_info["reordered"]
        Ks = eu.KrylovSubspace(np.float64, np.float64, N, m, 0, ctx)
        eu.arnoldi_(Ks, op, b, m=m, ishermitian=False)
        W = torch.full((k + 1, N), float("nan"), dtype=torch.float64, device="cuda").t()
        torch.cuda.synchronize()
        eu.phiv_(W, 0.5, Ks, k)
        res.append(_consume_on(torch, S, W)[0] if ctx is cA else W.cpu().numpy())
        del Ks
    close(res[0], ko.phiv(0.5, A, b, k, m=m), sc.TOL, "complete-on-return context, phiv! %s vs oracle" % entry)
    _late_output("phiv! (matrix output) " + entry, [res[1]], [res[0]])


def test_expv_batch_output_consumed_on_the_callers_stream(eu, torch, S, ctxs):
    cA, cP = ctxs("default", async_outputs=True)
    n, nprob, m = N, 5, 16
    rng = np.random.default_rng(n + 16)
    A0 = c2_operator(n).tocsr()
    A0.sort_indices()
    vals = np.stack([A0.data * s for s in (1 + 0.1 * rng.random(nprob))])
    B = np.asfortranarray(rng.standard_normal((n, nprob)))
    want = np.asarray(eu.expv_batch(0.8, A0, vals, B, m=m, ctx=cP))
    Bd = _colmajor(torch, B)
    torch.cuda.synchronize()
    W = eu.expv_batch(0.8, A0, vals, Bd, m=m, ctx=cA)
    got, = _consume_on(torch, S, W)
    _late_output("expv_batch", [got], [want])


def test_dense_outputs_consumed_on_the_callers_stream(eu, torch, S, ctxs):
    cA, cP = ctxs("default", async_outputs=True)
    A, k = _dense_inputs(130), 2
    wantE = eu.exponential_(_colmajor(torch, A), ctx=cP).cpu().numpy()
    wantP = [p.cpu().numpy() for p in eu.phi(_colmajor(torch, A), k, ctx=cP)]
    Ad, Ad2 = _colmajor(torch, A), _colmajor(torch, A)
    torch.cuda.synchronize()
    eu.exponential_(Ad, ctx=cA)
    phis = eu.phi(Ad2, k, ctx=cA)
    got = _consume_on(torch, S, Ad, *phis)
    _late_output("exponential!, phi!", got, [wantE] + wantP)


def test_two_calls_back_to_back_before_anything_is_consumed(eu, torch, S, ctxs):
    """two different calls of different sizes on the context before either output is read: the workspace and the internal
    KrylovSubspace are rebuilt under the first call's pending output"""
    cA, cP = ctxs("default", async_outputs=True)
    A1, A2 = sc.banded(N, np.float64), sc.banded(1537, np.float64)
    b1, b2 = sc.vector(N, np.float64, 0), sc.vector(1537, np.float64, 0)
    want = [np.asarray(eu.expv(T_STEP, eu.MIOperator(A1, cP), b1, m=20, ishermitian=False)),
            np.asarray(eu.phiv(0.5, eu.MIOperator(A2, cP), b2, 2, m=12, ishermitian=False))]
    op1, op2 = eu.MIOperator(A1, cA), eu.MIOperator(A2, cA)
    d1, d2 = torch.as_tensor(b1, device="cuda"), torch.as_tensor(b2, device="cuda")
    o1 = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eu.expv(T_STEP, op1, d1, m=20, ishermitian=False, out=o1)
    W2 = eu.phiv(0.5, op2, d2, 2, m=12, ishermitian=False)
    got = _consume_on(torch, S, o1, W2)
    _late_output("expv n=4100 then phiv n=1537, back to back", got, want)


def test_complete_on_return_outputs_on_a_callers_stream(eu, torch, S, ctxs):
    """async_outputs off on S: right after the call returns the output is complete for ANY reader -- the library's own copy to the host
    and a torch .cpu() issued on the default stream, which has no edge to S.  And with async_outputs on, HOST outputs are complete on
    return all the same."""
    cS, cP = ctxs("default")
    cA, _ = ctxs("default", async_outputs=True)
    A, b = sc.banded(N, np.float64), sc.vector(N, np.float64, 0)
    want = np.asarray(eu.expv(T_STEP, eu.MIOperator(A, cP), b, m=20, ishermitian=False))
    op = eu.MIOperator(A, cS)
    bd, out = torch.as_tensor(b, device="cuda"), torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eu.expv(T_STEP, op, bd, m=20, ishermitian=False, out=out)
    via_torch = out.cpu().numpy()
    via_lib = np.empty(N)
    eu.api._check(eu.api.L.load().expv_mi_memcpy_d2h(cS._h, via_lib.ctypes.data, out.data_ptr(), via_lib.nbytes), cS._h)
    _late_output("complete on return on S: .cpu(), expv_mi_memcpy_d2h", [via_torch, via_lib], [want, want])
    host = eu.expv(T_STEP, eu.MIOperator(A, cA), b, m=20, ishermitian=False)      # numpy in, numpy out: no synchronisation by the test
    _late_output("host output with async_outputs on", [np.asarray(host)], [want])


# ------------------------------------------------------------------------------------------- 4. ownership and the null stream
def test_the_callers_stream_outlives_the_context(eu, torch, S):
    A, b = sc.banded(N, np.float64), sc.vector(N, np.float64, 0)
    ctx = eu.Context(stream=S)
    op = eu.MIOperator(A, ctx)
    w = np.asarray(eu.expv(T_STEP, op, b, m=20, ishermitian=False))
    del op, ctx
    gc.collect()
    with torch.cuda.stream(S):
        x = torch.arange(1000, device="cuda", dtype=torch.float64)
        y = (x * 2).sum()
    S.synchronize()
    assert float(y) == 999000.0 and S.query()
    ctx2 = eu.Context(stream=S)                   # and the stream still carries a context
    assert np.array_equal(np.asarray(eu.expv(T_STEP, eu.MIOperator(A, ctx2), b, m=20, ishermitian=False)), w)


def test_two_contexts_share_one_stream(eu, S, ctxs):
    """two contexts on S (each with a helper stream, events and workspaces of its own), their calls interleaved: each result is the
    private stream's, bit for bit"""
    _, cP = ctxs("default")
    c1, c2 = eu.Context(stream=S), eu.Context(stream=S)
    A1, A2 = sc.banded(N, np.float64), sc.banded(1537, np.float64)
    b1, b2 = sc.vector(N, np.float64, 0), sc.vector(1537, np.float64, 0)
    want1 = np.asarray(eu.expv(T_STEP, eu.MIOperator(A1, cP), b1, m=20, ishermitian=False))
    want2 = np.asarray(eu.expv(T_STEP, eu.MIOperator(A2, cP), b2, m=12, ishermitian=False))
    o1, o2 = eu.MIOperator(A1, c1), eu.MIOperator(A2, c2)
    K1 = eu.KrylovSubspace(np.float64, np.float64, N, 20, 0, c1)
    eu.arnoldi_(K1, o1, b1, m=20, ishermitian=False, defer_tail=True)       # c1 has a closing pass pending ...
    g2 = np.asarray(eu.expv(T_STEP, o2, b2, m=12, ishermitian=False))         # ... while c2 works on the same stream
    g1 = np.asarray(eu.expv_(np.empty(N), T_STEP, K1))
    g1b = np.asarray(eu.expv(T_STEP, o1, b1, m=20, ishermitian=False))
    g2b = np.asarray(eu.expv(T_STEP, o2, b2, m=12, ishermitian=False))
    close(g1, ko.expv(T_STEP, A1, b1, m=20, ishermitian=False), sc.TOL, "two contexts on one stream: expv! of the subspace with the pending closing pass vs oracle")
    same = np.array_equal(g2, want2) and np.array_equal(g1b, want1) and np.array_equal(g2b, want2)
    REPORT.append(("shared_stream", "two contexts on S, calls interleaved", None, None, None, "bit-identical" if same else "DIFFERS"))
    assert same


def test_the_default_stream_is_refused(eu, torch):
    """Context(stream=torch.cuda.default_stream()): handle 0 is NULL for the C ABI, which would create a private stream in silence"""
    assert torch.cuda.default_stream().cuda_stream == 0
    with pytest.raises(ValueError, match="null / legacy stream"):
        eu.Context(stream=torch.cuda.default_stream())
    with pytest.raises(ValueError, match="None for a private stream"):
        eu.Context(stream=0)
