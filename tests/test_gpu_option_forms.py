"""Every option-selected form of the Krylov step against the oracle.

The context options (csrc/engine.h, struct Options) select about a dozen device code paths for one step; several of them are
the fallbacks the library takes by itself (an expired wait, a shape that does not fit).  The other GPU test files are thorough on
the DEFAULT form of each operator class; this file is the fixed table  forms x element types x calls x sizes:

* FORMS: (operator class, option set of tests/option_forms.py) -> the path words an expv through such a context reports.  A
  comparison that does not prove its form ran is worth nothing (with the options ignored it would still pass): every entry asserts
  the reported path of one expv exactly, and the context counters of every other call.
* element types Float64 / ComplexF64 / Float32 / ComplexF32; where an option does not apply to a type the table's function returns
  the path that DOES run, with the engine condition in a comment.
* calls: arnoldi full window (H entrywise, V max-abs), arnoldi iop = 3, Lanczos on the Hermitian part, expv real and complex t,
  phiv(k = 2, correct, errest), a continuation (init = m1), a happy breakdown inside the run, the deferred closing pass.
* sizes 513 / 4100 / 70001: one tile, a few tiles, many workgroups and a ragged last tile for the 8-byte and the 4-byte row packs.

Bars are the default form's own: 1e-12 for the 64-bit types (the oracle's own basis is asserted orthogonal to
1e-13, so no bar is widened by its loss of orthogonality); the fp32 bars of
test_native_32bit_single_pass_step / test_native_32bit_krylov_path (2e-5 expv, 3e-5 H and V, and the device within 20 x the distance
between the oracle run in 32-bit arithmetic and the fp64 oracle).  Each option set gets a private context, never the default one.
Every comparison prints the measured error next to its bar (tests/_util.close)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_oracle as ko
from tests._util import c2_operator, close
from tests.option_forms import OPTION_SETS, context_with

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


TYPES = (np.float64, np.complex128, np.float32, np.complex64)
SIZES = (513, 4100, 70_001)
DENSE_SIZES = (513, 1030, 2100)      # (a dense operator of 70 001 rows is 39 GB: the dense class crosses a tile boundary of the gemv blocks instead)


def _is32(T):
    return np.dtype(T).itemsize == (8 if np.dtype(T).kind == "c" else 4)


def _cplx(T):
    return np.dtype(T).kind == "c"


def _T64(T):
    return np.complex128 if _cplx(T) else np.float64


# ------------------------------------------------------------------ operator classes -----------------------------------------
def _banded(n, T, const):
    """the five-diagonal operator of test_native_32bit_single_pass_step: varying coefficients, or (const) one value per diagonal"""
    rng = np.random.default_rng(n)
    if const:
        A = c2_operator(n) * 0.5
    else:
        d = [0.3 + 0.1 * rng.random(n - 2), 1.2 + 0.1 * rng.random(n - 1), -1.0 + 0.1 * rng.random(n), 0.8 + 0.1 * rng.random(n - 1),
             -0.1 + 0.1 * rng.random(n - 2)]
        A = sp.diags(d, [-2, -1, 0, 1, 2], format="csr")
    if _cplx(T):
        A = A * (1 + 0.25j)
    return A.tocsr().astype(T)


def _grid(n, T, points):
    """2-D grid stencil (5- or 9-point, varying coefficients, no coupling across the ends of a grid row), rows of k cells; n is not a
    multiple of k: the last grid row is incomplete"""
    k = 64 if n < 60_000 else 200
    assert n % k != 0
    rng = np.random.default_rng(n + points)
    offs = [-k, -1, 0, 1, k] if points == 5 else [-k - 1, -k, -k + 1, -1, 0, 1, k - 1, k, k + 1]
    base = [0.7, 1.1, -4.0, 0.9, 1.3] if points == 5 else [0.2, 0.7, 0.25, 1.1, -4.0, 0.9, 0.15, 1.3, 0.3]
    i = np.arange(n)
    parts = []
    for o, c in zip(offs, base):
        ok = (i + o >= 0) & (i + o < n)
        ok &= np.abs((i + o) % k - i % k) <= 1            # a neighbour in the grid, not a wrap over the row end
        v = 0.25 * c * (1 + 0.1 * rng.random(n))
        if _cplx(T):
            v = v * (1 + 0.25j)
        parts.append(sp.csr_matrix((v[ok], (i[ok], i[ok] + o)), shape=(n, n)))
    A = sum(parts).tocsr()
    A.sort_indices()
    return A.astype(T)


def _random_rows(n, T):
    """five entries per row anywhere (the operator of tools/fa2_check.py): no single-pass form, the two-kernel step on SELL slots"""
    rng = np.random.default_rng(1)
    rows = np.repeat(np.arange(n), 5)
    cols = rng.integers(0, n, 5 * n)
    v = rng.standard_normal(5 * n) * 0.3
    if _cplx(T):
        v = v * (1 + 0.25j)
    A = (sp.csr_matrix((v, (rows, cols)), shape=(n, n)) - 0.5 * sp.eye(n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.astype(T)


def _powerlaw(n, T):
    from tests.test_gpu_parity import powerlaw_matrix
    A = powerlaw_matrix(n, 5, cplx=_cplx(T)).tocsr()
    A.sort_indices()
    return A.astype(T)


def _dense(n, T):
    rng = np.random.default_rng(n)
    A = -0.5 * np.eye(n) + (rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if _cplx(T) else 0)) / np.sqrt(n)
    return A.astype(T)


OPERATORS = {
    "banded": lambda n, T: _banded(n, T, False),
    "banded_const": lambda n, T: _banded(n, T, True),
    "grid5": lambda n, T: _grid(n, T, 5),
    "grid9": lambda n, T: _grid(n, T, 9),
    "random_rows": _random_rows,
    "powerlaw": _powerlaw,
    "dense": _dense,
}


def _hermitian_part(A64, T):
    S = (A64 + A64.conj().T) * 0.5
    return S.astype(T).tocsr() if sp.issparse(S) else S.astype(T)


def _with_invariant_block(A64, T):
    """rows and columns 0..5 cut off from the rest and replaced by an upper bidiagonal 6 x 6 block (the construction of
    test_overlapped_and_serial_pipeline_are_bitwise_identical inside the operator's own pattern: entries are dropped, the diagonal and
    the first super-diagonal of the block stay): a starting vector on the first 6 rows breaks down at step 6"""
    k = 6
    blk = np.diag(np.arange(1.0, k + 1) * 0.2 - 1.0) + np.diag(np.full(k - 1, 0.5), 1)
    if sp.issparse(A64):
        C = A64.tocoo()
        keep = (C.row >= k) & (C.col >= k)
        A2 = (sp.coo_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=C.shape)
              + sp.coo_matrix((blk[blk != 0], np.nonzero(blk)), shape=C.shape)).tocsr()
        A2.sort_indices()
        return A2.astype(T)
    A2 = np.array(A64)
    A2[:k, :] = 0
    A2[:, :k] = 0
    A2[:k, :k] = blk
    return A2.astype(T)


# ------------------------------------------------------------------ the oracle side, once per (operator class, type, size) ----
class Problem:
    def __init__(self, opclass, T, n):
        self.opclass, self.T, self.n = opclass, np.dtype(T), n
        self.T64 = np.dtype(_T64(T))
        self.single = _is32(T)
        self.m = 12 if _cplx(T) else 20            # complex windows: <= 15 columns on the single-pass step (pipe.hip)
        # happy breakdown = residual norm below `tol` (arnoldi.jl:370).  In 32-bit arithmetic the residual of an exactly invariant subspace is
        # a few eps_32 |A| ~ 1e-7 -- either side of the default tol = 1e-7, in the reference's Float32 methods too; the breakdown call of the
        # 32-bit types therefore passes tol = 1e-4 (far above that noise, far below the H[j+1, j] ~ 0.5 of the genuine steps) to both sides
        self.btol = 1e-4 if self.single else 1e-7
        rng = np.random.default_rng([n, 7])
        self.A = OPERATORS[opclass](n, T)
        self.A64 = self.A.astype(self.T64)          # the oracle sees exactly the values the device has
        self.b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if _cplx(T) else 0)).astype(T)
        self.b64 = self.b.astype(self.T64)
        self.S = _hermitian_part(self.A64, T)
        self.Abrk = _with_invariant_block(self.A64, T)
        self.bbrk = np.zeros(n, dtype=T)
        self.bbrk[:6] = (rng.standard_normal(6) + (1j * rng.standard_normal(6) if _cplx(T) else 0)).astype(T)
        self._memo = {}

    def oracle(self, what):
        """lazily: the oracle's subspace (and its loss of orthogonality) for one of the calls"""
        if what not in self._memo:
            m = self.m
            if what == "full":
                K = ko.arnoldi(self.A64, self.b64, m=m, ishermitian=False)
            elif what == "full32":                  # the oracle IN the 32-bit type: the scale of the fp32 bars
                K = ko.arnoldi(self.A, self.b, m=m, ishermitian=False)
            elif what == "iop3":
                K = ko.arnoldi(self.A64, self.b64, m=m, iop=3, ishermitian=False)
            elif what == "lanczos":
                K = ko.arnoldi(self.S.astype(self.T64), self.b64, m=m, ishermitian=True)
            elif what == "breakdown":
                K = ko.arnoldi(self.Abrk.astype(self.T64), self.bbrk.astype(self.T64), m=m, tol=self.btol, ishermitian=False)
            elif what == "phiv":
                self._memo[what] = ko.phiv(0.5, self.A64, self.b64, 2, m=m, correct=True, errest=True)
                return self._memo[what]
            V = np.asarray(K.getV())[:, : K.m + (0 if K.wasbreakdown else 1)].astype(np.complex128)
            loss = float(np.max(np.abs(V.conj().T @ V - np.eye(V.shape[1]))))
            # the 1e-12 bar presumes an oracle basis that is orthogonal to rounding: an operator change that spoils it is caught here, not
            # absorbed by a wider bar (iop = 3 is incomplete orthogonalisation by construction; the 32-bit types have their own fixed bars)
            assert what in ("iop3", "full32") or self.single or loss < 1e-13, (self.opclass, self.T.name, self.n, what, loss)
            self._memo[what] = (K, loss)
        return self._memo[what]

    def bar(self, which, loss=0.0):
        """the default form's bar (module docstring): fp32 fixed; 64-bit TOL = 1e-12 (`loss` is only asserted small, in oracle())"""
        if self.single:
            return {"w": 2e-5, "H": 3e-5, "V": 3e-5}[which]
        return 1e-12


@functools.lru_cache(maxsize=2)
def problem(opclass, Tname, n):
    return Problem(opclass, np.dtype(Tname), n)


# ------------------------------------------------------------------ the table of forms ----------------------------------------
# (operator class, option set) -> function (T, n) -> the exact set of path words (_lib.PATH_FLAGS) of an expv through that context.
PIPE = frozenset({"pipeline", "overlapped"})
PIPE_SERIAL = frozenset({"pipeline"})
TWO_KERNEL = frozenset({"two_kernel"})
MODULAR = frozenset({"modular"})


def _const(words):
    return lambda T, n: frozenset(words)


def _resident(T, n):
    # engine_core.hip: the resident kernel exists for Float64 only (`if constexpr (std::is_same<T, double>::value)`, a real, full-window,
    # non-augmented, fresh Arnoldi run on the diagonal form); every other type runs the overlapped step-wise form
    return PIPE | {"resident"} if np.dtype(T) == np.float64 else PIPE


def _banded_dia0(T, n):
    # choose_step_form: without a diagonal form the halo form of the single-pass step reads SELL slots, which exists for "the real
    # element types; everything else: DIA form only" (and creation builds no patch ordering for a band this narrow): the complex types
    # run the two-kernel step on SELL slots
    return PIPE if not _cplx(T) else TWO_KERNEL


def _grid_patch1(T, n):
    return PIPE | {"patch"}


def _grid_patch0(T, n):
    # wave form: `if constexpr (double || float)` -- the complex types have no wave form and a grid row is wider than the halo form's
    # reach (bandwidth > PIPE_WMAX): two-kernel step on the general diagonal form
    return frozenset({"pipeline", "wave", "overlapped"}) if not _cplx(T) else TWO_KERNEL


WAVE = frozenset({"pipeline", "wave", "overlapped"})


def _random_rows_default_step(T, n):
    # choose_step_form, `wave_sell`: creation records how many tiles the columns of a tile's rows reach over (Op::tile_reach), and
    # at these sizes (<= 400 tiles of 512 / 1024 rows) the real element types take the WAVE form of the single-pass step on SELL slots
    # (`if constexpr (double || float)`); the complex types have no wave form: two-kernel step.  fa2_pipelined and reorder are not what
    # decides here -- the *_pipeline0 sets are the ones that reach the two-kernel step's first kernel for the real types.
    return WAVE if not _cplx(T) else TWO_KERNEL


def _powerlaw_two_reductions(T, n):
    # choose_step_form: `stored = sell_ok && (single_red || sell_cut == 0)` -- rows cut at sell_cut + the overflow pass exist for the
    # single-reduction step only: the two-reduction variant leaves such an operator to the modular launches
    return MODULAR


FORMS = {}
for _o in ("default", "mailbox0", "nontemporal0", "nontemporal1"):
    FORMS[("banded", _o)] = _const(PIPE)
for _o in ("pipeline_serial", "mailbox0_pipeline_serial"):
    FORMS[("banded", _o)] = _const(PIPE_SERIAL)
FORMS[("banded", "dia0")] = _banded_dia0
FORMS[("banded", "resident")] = _resident
for _o in ("pipeline0", "pipeline0_dia0", "pipeline0_two_reductions"):
    FORMS[("banded", _o)] = _const(TWO_KERNEL)
FORMS[("banded", "pipeline0_fused0")] = _const(MODULAR)
FORMS[("banded_const", "default")] = _const(PIPE)
FORMS[("banded_const", "stencil")] = _const(PIPE)      # (the scalars replace the streamed diagonals for the real types, engine_core.hip `!ST<T>::is_complex && opt.stencil`; same path words)
for _g in ("grid5", "grid9"):
    FORMS[(_g, "patch1")] = FORMS[(_g, "patch1_mailbox0")] = _grid_patch1
    FORMS[(_g, "patch0")] = FORMS[(_g, "patch0_mailbox0")] = _grid_patch0
    FORMS[(_g, "patch0_wave0")] = FORMS[(_g, "patch0_wave0_mailbox0")] = _const(TWO_KERNEL)
for _r in ("random_rows", "powerlaw"):
    # (fa2_pipelined is read by the real element types' first kernel only, fused.hip; the complex types run the same two-kernel step either way)
    for _o in ("fa2_pipelined1_reorder0_pipeline0", "fa2_pipelined0_reorder0_pipeline0", "fa2_pipelined1_reorder0", "fa2_pipelined0_reorder0",
               "two_reductions", "reorder2"):
        FORMS[(_r, _o)] = _const(TWO_KERNEL)      # (powerlaw: rows cut at sell_cut + the overflow pass have no single-pass form)
    FORMS[(_r, "fused0")] = _const(MODULAR)
for _o in ("fa2_pipelined1_reorder0", "fa2_pipelined0_reorder0", "reorder2"):
    FORMS[("random_rows", _o)] = _random_rows_default_step
FORMS[("powerlaw", "two_reductions")] = _powerlaw_two_reductions
FORMS[("dense", "default")] = FORMS[("dense", "mailbox0")] = _const(MODULAR)

# The Lanczos call runs on the HERMITIAN PART of the class's operator -- another operator, whose stored form is its own.  Where that
# changes the step form the entry is here; everywhere else it is the class's form (the resident kernel is for Arnoldi: engine_core.hip
# `!lanczos`).  random_rows: (A + A') / 2 has 9 .. 11 entries per row at scattered columns -- rows of unequal length are cut at sell_cut
# and finished by the overflow pass, which has no single-pass form: two-kernel step for every type.
LANCZOS_FORMS = {("random_rows", _o): _const(TWO_KERNEL) for _o in ("fa2_pipelined1_reorder0", "fa2_pipelined0_reorder0", "reorder2")}
LANCZOS_FORMS[("random_rows", "two_reductions")] = _const(MODULAR)      # (cut rows + two reductions: the rule of _powerlaw_two_reductions)


def form_words(opclass, oset, T, n, lanczos=False):
    """the exact path words of an expv through (operator class, option set); lanczos: of the class's Hermitian part"""
    words = (LANCZOS_FORMS.get((opclass, oset), FORMS[(opclass, oset)]) if lanczos else FORMS[(opclass, oset)])(T, n)
    if lanczos:
        words = words - {"resident"}
    # "fa2_pipelined": the first kernel of the two-kernel step ran in its requests-up-front instantiation.  fused.hip, fused_a2: option
    # fa2_pipelined on, a real element type, a plain operator read from SELL SLOTS (the diagonal form is read instead when the operator
    # has one and `dia` is on, engine_core.hip `op.gndiag > 0 && c->opt.dia`), single reduction (the two-reduction step is another kernel)
    opts = OPTION_SETS[oset]
    sell_slots = opclass in ("random_rows", "powerlaw") or opts.get("dia", 1) == 0
    if "two_kernel" in words and not _cplx(T) and opts.get("fa2_pipelined", 1) and sell_slots and not opts.get("fused_two_reductions", 0):
        words = words | {"fa2_pipelined"}
    return words


def _cases():
    out = []
    for opclass in OPERATORS:
        osets = [o for (c, o) in FORMS if c == opclass]
        for n in (DENSE_SIZES if opclass == "dense" else SIZES):
            for T in TYPES:                       # (one oracle problem serves every option set of its class: kept adjacent for the cache)
                for o in osets:
                    out.append(pytest.param(opclass, o, T, n, id="%s-%s-%s-%d" % (opclass, o, np.dtype(T).name, n)))
    return out


def _counted(ctx, fn, nfact, words, label, whole_call=False):
    """run fn(); the context's counters must show nfact factorisations on the form `words` names, none of them redone"""
    c0 = ctx.counters()
    out = fn()
    c1 = ctx.counters()
    d = {k: c1[k] - c0[k] for k in c1}
    # (pipeline = 0 does not tell the two-kernel step from the modular launches, nor does frozenset() for the second part of a
    #  continuation on a wave form: for those forms the calls other than expv prove "not the single-pass step", the expv path is exact)
    # h_by_copy, the observable of `mailbox`: with the option on H comes home through the host mailbox (engine_core.hip, mailbox_arm)
    # from the overlapped single-pass forms, and from the single-reduction two-kernel step inside the whole-call expv (skip_tail:
    # steps_two_kernel fills the mailbox after its last step); every other form and call copies and synchronises
    by_mailbox = ctx.get_option("mailbox") == 1 and (
        "overlapped" in words or (whole_call and "two_kernel" in words and not ctx.get_option("fused_two_reductions")))
    want = {"factorisations": nfact, "pipeline": nfact if "pipeline" in words else 0,
            "overlapped": nfact if "overlapped" in words else 0, "redo_serial": 0, "redo_wave_off": 0,
            "h_by_copy": 0 if by_mailbox else nfact}
    got = {k: d[k] for k in want}
    assert got == want, "%s: counters %r, expected %r" % (label, got, want)
    return out


def _expv_path(eu, t, op, b, **kw):
    w = eu.expv(t, op, b, **kw)
    st = eu.expv.last_stats      # (the step form's words + which first kernel the two-kernel step ran, reported beside them)
    return np.asarray(w), frozenset(st["path"]) | ({"fa2_pipelined"} if st["fa2_pipelined"] else frozenset())


@pytest.mark.parametrize("opclass,oset,T,n", _cases())
def test_option_form_matches_oracle(eu, opclass, oset, T, n):
    """One (operator class, option set, element type, size): every call of the module docstring against the oracle at the default
    form's bar, with the path / counters that prove the form ran."""
    P = problem(opclass, np.dtype(T).name, n)
    m, T64 = P.m, P.T64
    words = form_words(opclass, oset, T, n)
    ctx = context_with(eu, OPTION_SETS[oset])
    op = eu.MIOperator(P.A, ctx)                       # (after the options: dia / patch / reorder / stencil act at creation)
    tag = "%s/%s %s n=%d" % (opclass, oset, np.dtype(T).name, n)
    as64 = lambda x: np.asarray(x).astype(T64)

    # expv, real t: the path words, then the result
    Ko, loss = P.oracle("full")
    w, path = _expv_path(eu, 0.6, op, P.b, m=m, ishermitian=False)
    print("[path] %-90s %s" % (tag + ": expv", "+".join(sorted(path))))
    assert path == words, "%s: expv ran on %s, the table says %s" % (tag, sorted(path), sorted(words))
    assert w.dtype == np.dtype(T)
    close(as64(w), ko.expv_(np.empty(n, dtype=T64), 0.6, Ko), P.bar("w", loss), "%s: expv" % tag)
    # expv, complex t
    wc = _counted(ctx, lambda: eu.expv(0.3 - 0.4j, op, P.b, m=m, ishermitian=False), 1, words, tag + " expv complex t", whole_call=True)
    close(np.asarray(wc).astype(np.complex128), ko.expv_(np.empty(n, dtype=np.complex128), 0.3 - 0.4j, Ko), P.bar("w", loss),
          "%s: expv complex t" % tag)

    # arnoldi, full window: H entrywise, V max-abs
    Ks = _counted(ctx, lambda: eu.arnoldi(op, P.b, m=m, ishermitian=False), 1, words, tag + " arnoldi")
    assert Ks.m == Ko.m and bool(Ks.wasbreakdown) == bool(Ko.wasbreakdown)
    eH = close(as64(Ks.getH()), Ko.getH(), P.bar("H", loss), "%s: arnoldi H" % tag, mat=True)
    eV = close(as64(Ks.getV()), Ko.getV(), P.bar("V", loss), "%s: arnoldi V (max abs)" % tag, absolute=True)
    if P.single:
        K32, _ = P.oracle("full32")
        rH = float(np.max(np.abs(as64(K32.getH()) - Ko.getH())) / np.max(np.abs(Ko.getH())))
        rV = float(np.max(np.abs(as64(K32.getV()) - Ko.getV())))
        print("[parity] %-90s H %.3e  V %.3e" % ("  the oracle in %s arithmetic vs the fp64 oracle" % np.dtype(T).name, rH, rV))
        assert eH <= 20 * rH + 1e-7 and eV <= 20 * rV + 1e-7, (tag, eH, rH, eV, rV)

    # arnoldi, incomplete orthogonalisation over a window of 3
    Ko3, loss3 = P.oracle("iop3")
    K3 = _counted(ctx, lambda: eu.arnoldi(op, P.b, m=m, iop=3, ishermitian=False), 1, words - {"resident"}, tag + " arnoldi iop=3")
    assert K3.m == Ko3.m
    close(as64(K3.getH()), Ko3.getH(), P.bar("H"), "%s: arnoldi iop=3 H" % tag, mat=True)
    close(as64(K3.getV()), Ko3.getV(), P.bar("V"), "%s: arnoldi iop=3 V (max abs)" % tag, absolute=True)

    # Lanczos on the Hermitian part
    KoL, lossL = P.oracle("lanczos")
    opS = eu.MIOperator(P.S, ctx)
    wordsL = form_words(opclass, oset, T, n, lanczos=True)
    _, pathL = _expv_path(eu, 0.6, opS, P.b, m=m, ishermitian=True)
    print("[path] %-90s %s" % (tag + ": expv, Hermitian part (Lanczos)", "+".join(sorted(pathL))))
    assert pathL == wordsL, "%s: Lanczos on the Hermitian part ran on %s, the table says %s" % (tag, sorted(pathL), sorted(wordsL))
    KL = _counted(ctx, lambda: eu.arnoldi(opS, P.b, m=m, ishermitian=True), 1, wordsL, tag + " Lanczos")
    assert KL.m == KoL.m and KL.U == np.dtype(np.float32 if P.single else np.float64)
    close(np.asarray(KL.getH()).astype(np.float64), np.real(KoL.getH()), P.bar("H", lossL), "%s: Lanczos H" % tag, mat=True)
    close(as64(KL.getV()), KoL.getV(), P.bar("V", lossL), "%s: Lanczos V (max abs)" % tag, absolute=True)

    # phiv with the corrected last column and the error estimate
    Wo, esto = P.oracle("phiv")
    (W, est) = _counted(ctx, lambda: eu.phiv(0.5, op, P.b, 2, m=m, ishermitian=False, correct=True, errest=True), 1, words, tag + " phiv")
    close(as64(W), Wo, P.bar("w", loss), "%s: phiv k=2 correct" % tag)
    print("[parity] %-90s device %.6e  oracle %.6e" % (tag + ": phiv error estimate", est, esto))
    assert np.isfinite(est)
    if not P.single and esto > 1e-10 * float(np.linalg.norm(Wo)):
        close(est, esto, 1e-6, "%s: phiv error estimate (relative; where it is more than rounding noise)" % tag)

    # continuation: m1 steps, then init = m1 up to m  (a wave form needs a fresh call and two reductions have no continuation:
    # choose_step_form `if (!fresh)` -- those continue on the two-kernel step / the modular launches)
    m1 = m // 2
    Kc = eu.KrylovSubspace(T, T, n, m, 0, ctx)
    _counted(ctx, lambda: eu.arnoldi_(Kc, op, P.b, m=m1, ishermitian=False), 1, words, tag + " continuation, first part")
    assert not Kc.wasbreakdown
    cwords = words if "wave" not in words else frozenset()
    _counted(ctx, lambda: eu.arnoldi_(Kc, op, P.b, m=m, ishermitian=False, init=m1), 1, cwords - {"resident"}, tag + " continuation, second part")
    close(as64(Kc.getH()), Ko.getH(), P.bar("H", loss), "%s: continuation %d -> %d H" % (tag, m1, m), mat=True)
    close(as64(Kc.getV()), Ko.getV(), P.bar("V", loss), "%s: continuation %d -> %d V (max abs)" % (tag, m1, m), absolute=True)

    # happy breakdown inside the run
    Kob, lossb = P.oracle("breakdown")
    opb = eu.MIOperator(P.Abrk, ctx)
    _, pathb = _expv_path(eu, 0.6, opb, P.bbrk, m=m, tol=P.btol, ishermitian=False)
    print("[path] %-90s %s" % (tag + ": expv, operator with the invariant block", "+".join(sorted(pathb))))
    assert pathb == words, "%s: the operator with the invariant block ran on %s, the table says %s" % (tag, sorted(pathb), sorted(words))
    Kb = _counted(ctx, lambda: eu.arnoldi(opb, P.bbrk, m=m, tol=P.btol, ishermitian=False), 1, words, tag + " breakdown")
    assert (Kb.m, bool(Kb.wasbreakdown)) == (Kob.m, bool(Kob.wasbreakdown)) and Kob.wasbreakdown and Kob.m == 6, (tag, Kb.m, Kb.wasbreakdown, Kob.m)
    mb = Kob.m
    close(as64(Kb.getH())[: mb + 1, :mb], Kob.getH()[: mb + 1, :mb], P.bar("H", lossb), "%s: breakdown at step %d, H" % (tag, mb), mat=True)
    close(as64(Kb.getV())[:, :mb], Kob.getV()[:, :mb], P.bar("V", lossb), "%s: breakdown at step %d, V (max abs)" % (tag, mb), absolute=True)
    close(as64(eu.expv_(np.empty(n, dtype=T), 0.6, Kb)), ko.expv_(np.empty(n, dtype=T64), 0.6, Kob), P.bar("w", lossb), "%s: breakdown, expv!" % tag)

    # deferred closing pass: what the undeferred call OF THE SAME FORM gives, bit for bit, whoever collects it
    def fresh(defer):
        K = eu.KrylovSubspace(T, T, n, m + 2, 0, ctx)
        eu.arnoldi_(K, op, P.b, m=m, ishermitian=False, defer_tail=defer)
        return K
    K0 = fresh(False)
    H0 = np.asarray(K0.getH()).copy()
    w0 = np.asarray(eu.expv_(np.empty(n, dtype=T), 0.4, K0)).copy()
    V0 = np.asarray(K0.getV()).copy()
    Kd = fresh(True)
    assert np.array_equal(np.asarray(Kd.getH()), H0), tag + ": deferred closing pass, getH first"
    assert np.array_equal(np.asarray(Kd.getV()), V0), tag + ": deferred closing pass, getV after getH"
    Kd = fresh(True)
    assert np.array_equal(np.asarray(eu.expv_(np.empty(n, dtype=T), 0.4, Kd)), w0), tag + ": deferred closing pass, expv! first"
    assert np.array_equal(np.asarray(Kd.getH()), H0) and np.array_equal(np.asarray(Kd.getV()), V0), tag + ": deferred closing pass, after expv!"
    c = ctx.counters()
    assert c["redo_serial"] == 0 and c["redo_wave_off"] == 0, c


# ------------------------------------------------------------------ bit-for-bit pairs ------------------------------------------
def _products(eu, P, oset):
    """H, V, w of the calls whose arithmetic the pair's option must not change"""
    ctx = context_with(eu, OPTION_SETS[oset])
    T, n, m = P.T, P.n, P.m
    op = eu.MIOperator(P.A, ctx)
    out = {}
    w, path = _expv_path(eu, 0.6, op, P.b, m=m, ishermitian=False)
    out["expv w"] = w.copy()
    for name, o, b, kw in (("full", op, P.b, dict(ishermitian=False)), ("iop3", op, P.b, dict(iop=3, ishermitian=False)),
                           ("lanczos", eu.MIOperator(P.S, ctx), P.b, dict(ishermitian=True)),
                           ("breakdown", eu.MIOperator(P.Abrk, ctx), P.bbrk, dict(tol=P.btol, ishermitian=False))):
        K = eu.arnoldi(o, b, m=m, **kw)
        out[name + " m"] = np.array([K.m, int(K.wasbreakdown)])
        H, mk = np.asarray(K.getH()).copy(), int(K.m)
        out[name + " w"] = np.asarray(eu.expv_(np.empty(n, dtype=T), 0.6, K)).copy()
        V = np.asarray(K.getV())
        out[name + " V"] = V[:, :mk].copy()
        if not K.wasbreakdown:      # the two outputs of the CLOSING pass, kept apart: H[m+1, m] and v_{m+1}
            out[name + " tail H[m+1, m]"] = H[mk, mk - 1].copy()
            out[name + " tail v_{m+1}"] = V[:, mk].copy()
            H[mk, mk - 1] = 0
        out[name + " H"] = H
    c = ctx.counters()
    assert c["redo_serial"] == 0 and c["redo_wave_off"] == 0, c
    return out, path


# stated by the project (its own tests assert them for Float64): a pair that is not bit-identical for some type is a finding
STATED_PAIRS = [("banded", "default", "pipeline_serial"), ("banded", "mailbox0", "mailbox0_pipeline_serial"),
                ("banded", "nontemporal0", "nontemporal1"), ("banded_const", "default", "stencil")]
# expected from the code, recorded nowhere before this file: measured once, then pinned (see the test's docstring)
EXPECTED_PAIRS = [("banded", "default", "mailbox0"), ("grid5", "patch1", "patch1_mailbox0"), ("grid9", "patch0", "patch0_mailbox0"),
                  ("grid5", "patch0_wave0", "patch0_wave0_mailbox0"), ("dense", "default", "mailbox0"),
                  ("random_rows", "fa2_pipelined1_reorder0_pipeline0", "fa2_pipelined0_reorder0_pipeline0"),
                  ("powerlaw", "fa2_pipelined1_reorder0_pipeline0", "fa2_pipelined0_reorder0_pipeline0"),
                  ("powerlaw", "fa2_pipelined1_reorder0", "fa2_pipelined0_reorder0")]


def _pair_cases(pairs):
    return [pytest.param(c, a, b, T, n, id="%s-%s-vs-%s-%s-%d" % (c, a, b, np.dtype(T).name, n))
            for (c, a, b) in pairs for n in (DENSE_SIZES if c == "dense" else SIZES) for T in TYPES]


def _assert_pair_bitwise(eu, opclass, a, b, T, n, tail_ulps=0):
    """every product of the pair equal bit for bit; with tail_ulps > 0 the two outputs of the closing pass are held to that many units
    in the last place of the storage type (relative to the largest entry) instead"""
    P = problem(opclass, np.dtype(T).name, n)
    (ra, pa), (rb, pb) = _products(eu, P, a), _products(eu, P, b)
    assert pa == form_words(opclass, a, T, n) and pb == form_words(opclass, b, T, n), (a, sorted(pa), b, sorted(pb))
    worst = {}
    ulp = float(np.finfo(np.dtype(T)).eps)
    for k in ra:
        if tail_ulps and " tail " in k:
            close(ra[k], rb[k], tail_ulps * ulp, "%s %s vs %s, %s n=%d: %s (units of eps: %d)" % (opclass, a, b, np.dtype(T).name, n, k, tail_ulps),
                  mat=True)
            continue
        if not np.array_equal(ra[k], rb[k]):      # (what differs, by how much, in how many entries and in which columns)
            ne = ra[k] != rb[k]
            worst[k] = (float(np.max(np.abs(ra[k].astype(np.complex128) - rb[k].astype(np.complex128)))), int(ne.sum()),
                        sorted(set(np.nonzero(ne)[-1].tolist())) if ne.ndim == 2 else None, ra[k].shape)
    assert not worst, "%s %s vs %s, %s n=%d: not bit-identical, max abs differences %r" % (opclass, a, b, np.dtype(T).name, n, worst)
    return pa, pb


@pytest.mark.parametrize("opclass,a,b,T,n", _pair_cases(STATED_PAIRS))
def test_stated_bitwise_pairs_hold_for_every_element_type(eu, opclass, a, b, T, n):
    """Pairs the project states to be bit-identical -- overlapped vs one launch after the other (with and without the mailbox),
    non-temporal loads off / on, the constant-coefficient stencil off / on -- on H, V and w of the full window, the IOP window,
    Lanczos and a mid-run breakdown, now for all four element types (the older tests assert them for Float64).

    Finding of this test's first run: overlapped vs one-launch-after-the-other is bit-identical on H[1:m, 1:m], V[:, 1:m] and w for
    every type, size and call here, but NOT always on the (m+1)-th column: Float64 n = 4100 (full window: H[m+1, m] off by 2.2e-16,
    v_{m+1} by 1.4e-17 in 3712 rows) and Float32 n = 513 (Lanczos: v_{m+1} by 1.5e-8 = one unit in the last place, 391 rows).  The claim
    was too wide, no kernel is wrong: steps 1..m are the same kernel in both forms, but v_{m+1} and H[m+1, m] come from the closing
    pass (pipe.hip) in the overlapped form and from update2 + norm_final (engine_core.hip, steps_single_pass) in the other -- two
    reductions of the same n squares with another grouping of the partial sums, so beta_m may differ in its last bit and v_{m+1} =
    u / beta_m with it.  The pair is therefore pinned bit for bit on everything the m steps produce, and the closing pass's two
    outputs are held to 4 units in the last place of the storage type (two roundings of a sum, a square root, a division; measured: 1)
    -- DESIGN.md section 5 says the same now.  The other stated pairs stay bit-identical including that column."""
    pa, pb = _assert_pair_bitwise(eu, opclass, a, b, T, n, tail_ulps=4 if "pipeline_serial" in b else 0)
    if "pipeline_serial" in b:
        assert "overlapped" in pa and "overlapped" not in pb, (pa, pb)      # (the pair really is the two hand-overs)


@pytest.mark.parametrize("opclass,a,b,T,n", _pair_cases(EXPECTED_PAIRS))
def test_expected_bitwise_pairs(eu, opclass, a, b, T, n):
    """Pairs expected to be bit-identical from the code and recorded nowhere before: `mailbox` 0 / 1 (only the way H comes home
    differs, engine_core.hip mailbox_arm / read_back) on the banded, patch, wave, two-kernel and modular forms, and `fa2_pipelined`
    0 / 1 (the same products and sums with the loads issued earlier, fused.hip; the complex types do not read the option).  That the
    two members really ran differently is asserted, not assumed: the path word `fa2_pipelined` is present on one side only for the real
    types (form_words), and the mailbox members differ in the `h_by_copy` counter of test_option_form_matches_oracle, where both members
    of every pair are also compared with the oracle."""
    _assert_pair_bitwise(eu, opclass, a, b, T, n)


# ------------------------------------------------------------------ kiops_skip_redo --------------------------------------------
KIOPS_N = 70_001


@functools.lru_cache(maxsize=1)
def _kiops_inputs():
    n = KIOPS_N
    rng = np.random.default_rng(21)
    A = c2_operator(n)
    u = rng.standard_normal((n, 3)) * 50
    u2 = rng.standard_normal((n, 3)) * 50
    return {False: (A, u), True: ((A * (1 + 0.25j)).tocsr(), u + 1j * u2)}


KIOPS_KW = {"iop2_tol1e-10": dict(iop=2, tol=1e-10), "iop3_m12": dict(iop=3, m=12)}
KIOPS_STATS = {(False, "iop2_tol1e-10"): (1, 2, 0, 3, 25), (False, "iop3_m12"): (1, 1, 0, 2, 21),
               (True, "iop2_tol1e-10"): (1, 2, 0, 3, 26), (True, "iop3_m12"): (1, 1, 0, 2, 22)}


@functools.lru_cache(maxsize=4)
def _kiops_oracle(cplx, kwname):
    A, u = _kiops_inputs()[cplx]
    return ko.kiops(2.0, A, u, allow_complex=cplx, ishermitian=False, **KIOPS_KW[kwname])


@pytest.mark.parametrize("base", ["default", "mailbox0", "pipeline_serial", "pipeline0"])
@pytest.mark.parametrize("kwname", list(KIOPS_KW))
@pytest.mark.parametrize("cplx", [False, True], ids=["float64", "complex128"])
def test_kiops_skip_redo_both_ways(eu, cplx, kwname, base):
    """ADVICE, first finding: kiops after a REJECTED sub-step either continues behind the closing pass (kiops_skip_redo = 1,
    init = j + 1) or recomputes step j like the reference's loop (0).  Inputs whose every run contains rejections (asserted first:
    without one nothing is tested); both settings give the oracle's statistics and its w at 1e-12.  Also where the deferral behind
    skip_redo is off (no mailbox, one launch after the other) and on the two-kernel step (pipeline = 0).

    Measured on the first run: the two w are NOT equal bit for bit -- they differ in the last bit of a few entries (max abs 7.1e-15 ..
    5.7e-14 on entries of size 10 .. 100; relative 2-norm difference 4e-19 .. 7e-18, all sixteen combinations).  Reason: the recomputed
    step j does not have bit-identical inputs after all.  With kiops_skip_redo = 0 column j of H and v_{j+1} are produced again by the
    FIRST pass of a continuation (which takes v_init as already normalised and projects on the stored window), with 1 they are what the
    closing pass of the previous call left (un-normalised column and its scale): the same projection sums in another order.  Both are
    held to the oracle at 1e-12 and to each other at the same bar; the recomputing run takes 1 .. 2 Krylov steps more."""
    A, u = _kiops_inputs()[cplx]
    wo, so = _kiops_oracle(cplx, kwname)
    assert so[1] >= 1, so
    assert tuple(so) == KIOPS_STATS[(cplx, kwname)], so
    res = []
    for skip in (0, 1):
        ctx = context_with(eu, dict(OPTION_SETS[base], kiops_skip_redo=skip))
        op = eu.MIOperator(A, ctx)
        c0 = ctx.counters()
        w, st = eu.kiops(2.0, op, u, allow_complex=cplx, ishermitian=False, **KIOPS_KW[kwname])
        c1 = ctx.counters()
        d = {k: c1[k] - c0[k] for k in c1}
        want_pipe = 0 if base == "pipeline0" else d["factorisations"]
        assert d["factorisations"] >= 2 and d["pipeline"] == want_pipe and d["redo_serial"] == 0 and d["redo_wave_off"] == 0, (base, skip, d)
        assert d["overlapped"] == (d["factorisations"] if base in ("default", "mailbox0") else 0), (base, skip, d)
        assert d["h_by_copy"] == (0 if base == "default" else d["factorisations"]), (base, skip, d)      # (the mailbox: overlapped steps + option on)
        assert tuple(st) == tuple(so), (base, skip, st, so)
        close(w, wo, 1e-12, "kiops %s %s on %s, kiops_skip_redo=%d vs oracle" % ("complex128" if cplx else "float64", kwname, base, skip))
        res.append((np.asarray(w).copy(), d["krylov_steps"]))
    close(res[1][0], res[0][0], 1e-12, "kiops %s %s on %s: kiops_skip_redo=1 vs 0" % ("complex128" if cplx else "float64", kwname, base))
    print("[counters] krylov steps: recomputed %d, skipped %d" % (res[0][1], res[1][1]))
    assert res[1][1] < res[0][1]                           # (every run here has a rejection: the recomputing loop takes at least one step more)


# ------------------------------------------------------------------ batch_rounds -----------------------------------------------
@functools.lru_cache(maxsize=1)
def _batch_problem(Tname, n):
    T = np.dtype(Tname)
    cplx = T.kind == "c"
    T64 = np.dtype(_T64(T))
    rng = np.random.default_rng(n + 16)
    nprob, m = 16, 12 if cplx else 16
    A0 = (c2_operator(n) * ((1 + 0.25j) if cplx else 1.0)).tocsr()
    A0.sort_indices()
    A0 = A0.astype(T)
    vals = np.stack([A0.data * s for s in (1 + 0.1 * rng.random(nprob))]).astype(T)
    B = np.asfortranarray((rng.standard_normal((n, nprob)) + (1j * rng.standard_normal((n, nprob)) if cplx else 0)).astype(T))
    Wo = np.empty((n, nprob), dtype=T64)
    for p in range(nprob):
        Ap = A0.astype(T64).copy()
        Ap.data = vals[p].astype(T64)
        Wo[:, p] = ko.expv(0.8, Ap, B[:, p].astype(T64), m=m, ishermitian=False)
    return A0, vals, B, Wo, m


@pytest.mark.parametrize("oset", ["batch_rounds1", "default", "batch_rounds3", "batch_rounds7", "pipeline0"])
@pytest.mark.parametrize("nprob", [5, 16])
@pytest.mark.parametrize("T", [np.float64, np.complex128, np.float32])
@pytest.mark.parametrize("n", [4100, 70_001])
def test_batch_rounds(eu, n, T, nprob, oset):
    """expv_batch on the banded pattern with the batched single-pass step's resident rounds set to 1, 2 (default), 3 and 7 -- pipe.hip
    turns the value into tiles per workgroup by a rounded-up division, the odd values are where a last workgroup gets fewer -- and on
    the batched two-kernel step (pipeline = 0): every column against the oracle's single-problem expv at the bars of
    test_expv_batch_matches_single_problem_loop / test_expv_batch_other_element_types (1e-12; 3e-5 for Float32).
    Known limit: the value ends as a launch geometry and nothing of it comes back to the host, so that it was READ shows only through
    get_option -- a wrong geometry fails the oracle comparison here, an ignored value would not."""
    A0, vals, B, Wo, m = _batch_problem(np.dtype(T).name, n)
    ctx = context_with(eu, OPTION_SETS[oset])
    assert ctx.get_option("batch_rounds") == OPTION_SETS[oset].get("batch_rounds", 2)
    W, mu = eu.expv_batch(0.8, A0, vals[:nprob], np.asfortranarray(B[:, :nprob]), m=m, ctx=ctx, return_m=True)
    assert np.asarray(W).dtype == np.dtype(T) and all(int(x) == m for x in mu)
    tol = 3e-5 if _is32(T) else 1e-12
    for p in range(nprob):
        close(np.asarray(W)[:, p].astype(Wo.dtype), Wo[:, p], tol, "expv_batch %s n=%d, %d problems, %s: problem %d vs the oracle's expv"
              % (np.dtype(T).name, n, nprob, oset, p))


# ------------------------------------------------------------------ state after a failed call ----------------------------------
def _poisoned(eu, A, ctx):
    """an operator of A's size, type and pattern with one NaN among its values"""
    A2 = A.copy()
    A2.data = A2.data.copy()
    A2.data[A2.nnz // 2] = np.nan
    try:
        op = eu.MIOperator(A.copy(), ctx)
        op.update_values(A2)
        return op, None
    except Exception:          # (creation or the update refuses non-finite values: the NaN goes into the input vector instead)
        return eu.MIOperator(A, ctx), "vector"


def _returns(fn):
    try:
        fn()
    except Exception as e:     # the library's error (non-finite H in the host exponential) or non-finite numbers: either is fine
        return type(e).__name__
    return None


@pytest.mark.parametrize("cplx", [False, True], ids=["float64", "complex128"])
def test_kiops_after_a_failed_call_on_the_same_context(eu, cplx):
    """ADVICE, second finding: kiops asks for a deferred closing pass and collects it after the host exponential; when that throws
    (non-finite H) the pass stayed pending on the workspace the context keeps between calls, and the next call's first factorisation
    wrote the failed call's H[m+1, m], column scale and breakdown flag into the fresh subspace.  After a call on a poisoned operator
    -- whatever it does -- the same context must give what a fresh context gives, bit for bit, with the oracle's statistics."""
    A, u = _kiops_inputs()[cplx]
    kw = dict(allow_complex=cplx, ishermitian=False, **KIOPS_KW["iop2_tol1e-10"])
    wo, so = _kiops_oracle(cplx, "iop2_tol1e-10")
    ctx = eu.Context()
    bad, how = _poisoned(eu, A, ctx)
    ubad = u
    if how == "vector":
        ubad = u.copy()
        ubad[KIOPS_N // 2, 0] = np.nan
    raised = _returns(lambda: eu.kiops(2.0, bad, ubad, **kw))
    print("[state] kiops on the poisoned %s: %s" % (how or "operator", raised or "returned"))
    w, st = eu.kiops(2.0, eu.MIOperator(A, ctx), u, **kw)
    assert tuple(st) == tuple(so), (st, so)
    close(w, wo, 1e-12, "kiops after a failed call on the same context (%s) vs oracle" % ("complex128" if cplx else "float64"))
    ctx2 = eu.Context()
    w2, st2 = eu.kiops(2.0, eu.MIOperator(A, ctx2), u, **kw)
    assert tuple(st2) == tuple(st) and np.array_equal(np.asarray(w), np.asarray(w2))
    c = ctx.counters()
    assert c["redo_serial"] == 0 and c["redo_wave_off"] == 0, c


@pytest.mark.parametrize("through", ["work_set", "caches"])
def test_adaptive_timestep_after_a_failed_call_on_the_same_context(eu, through):
    """The adaptive time stepper defers the closing pass the same way (engine_drivers.hip, `factorise`) on the work set the context
    keeps (expv_timestep without caches) or on the caller's caches (phiv_timestep! with caches=): a failed call must leave neither in
    a state the next call can see."""
    n = KIOPS_N
    A = c2_operator(n)
    rng = np.random.default_rng(22)
    ts = np.array([0.4, 1.0])
    kw = dict(adaptive=True, tol=1e-8, m=20)
    if through == "work_set":
        B = rng.standard_normal(n)
    else:
        B = np.asfortranarray(rng.standard_normal((n, 3)))

    def run(ctx, M, Bx, caches, stats=None):
        U = np.empty((n, len(ts)), dtype=np.float64, order="F")
        if through == "work_set":
            return np.asarray(eu.expv_timestep(ts.copy(), M, Bx, stats=stats, **kw))
        return np.asarray(eu.phiv_timestep_(U, ts.copy(), M, Bx, caches=caches, stats=stats, **kw))
    ctx = eu.Context()
    caches = eu.timestep_caches(B if B.ndim == 1 else B[:, 0], 40, 2, ctx) if through == "caches" else None
    bad, how = _poisoned(eu, A, ctx)
    Bbad = B
    if how == "vector":
        Bbad = B.copy()
        Bbad[(n // 2,) + (0,) * (B.ndim - 1)] = np.nan
    raised = _returns(lambda: run(ctx, bad, Bbad, caches))
    print("[state] adaptive time stepper (%s) on the poisoned %s: %s" % (through, how or "operator", raised or "returned"))
    st, so = {}, {}
    U = run(ctx, eu.MIOperator(A, ctx), B, caches, st)
    Uo = ko.phiv_timestep(ts.copy(), A, B, stats=so, **kw)
    assert (st["num_timesteps"], st["matvecs"], st["m"]) == (so["num_timesteps"], so["matvecs"], so["m"]), (st, so)
    close(U, Uo, 1e-12, "adaptive time stepper (%s) after a failed call on the same context vs oracle" % through)
    ctx2 = eu.Context()
    caches2 = eu.timestep_caches(B if B.ndim == 1 else B[:, 0], 40, 2, ctx2) if through == "caches" else None
    U2 = run(ctx2, eu.MIOperator(A, ctx2), B, caches2)
    assert np.array_equal(U, U2)


# ------------------------------------------------------------------ a subspace that outlives its context ------------------------
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_subspace_of_a_reordered_operator_may_outlive_its_context(eu, T):
    """Found by this file's first runs (a process abort inside an unrelated allocation, tests later): a fresh factorisation through a
    REORDERED operator on the two-kernel step or the modular launches keeps the permuted starting vector in Ks.b_stored, a buffer
    taken from the context's staging spares -- and a KrylovSubspace destroyed AFTER its context (any finaliser order is legal: Julia's
    GC, Python's cycle collector after a failed test) handed it back to the freed context: a write into freed host memory.  The
    sequence itself, finalisers in that order, with allocations and library calls behind it.  (Heap damage need not show at once;
    this pins the sequence, the fix is in ~Ks.)"""
    P = problem("random_rows", np.dtype(T).name, 4100)
    for oset in ("reorder2", "fused0"):
        ctx = context_with(eu, dict(OPTION_SETS[oset], pipeline=0))
        op = eu.MIOperator(P.A, ctx)
        assert op.reorder_info["reordered"] if oset == "reorder2" else True
        Ks = eu.KrylovSubspace(T, T, P.n, P.m, 0, ctx)
        eu.arnoldi_(Ks, op, P.b, m=P.m, ishermitian=False)
        H = np.asarray(Ks.getH()).copy()
        ctx._finalizer()            # the context first ...
        Ks._finalizer()             # ... then the handles that pointed at it
        op._finalizer()
        junk = [np.empty(k * 97 + 1) for k in range(200)]      # the allocator walks its free lists
        del junk
        ctx2 = context_with(eu, OPTION_SETS[oset])
        K2 = eu.arnoldi(eu.MIOperator(P.A, ctx2), P.b, m=P.m, ishermitian=False)
        Ko, loss = P.oracle("full")
        close(np.asarray(K2.getH()).astype(P.T64), Ko.getH(), P.bar("H", loss), "arnoldi H after a context was destroyed before its subspace (%s, %s)"
              % (oset, np.dtype(T).name), mat=True)
        assert np.isfinite(H).all()
