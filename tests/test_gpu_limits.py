"""One call on each side of every compiled-in capacity limit (tests/limits.py reads them from csrc/kernels.h).

The engine compares a call against these constants to pick a Krylov step form, a combine kernel, a reduction shape; each constant also
sizes an LDS array, an array inside the kernel arguments or a bit field.  An off-by-one in the last slot of such an array does not
fault -- it reads a neighbour and gives a wrong number -- and one past the limit another kernel runs.  The rest of the suite sits well
inside the limits; here every boundary value is computed from LIMITS, every case is compared with the oracle at the default form's bar
and proves which side it ran on: the path words of expv.last_stats, the context counters, per-kernel launch counts of
Context.prof_get() where a driver reports no path.  Where nothing observable separates the sides (the combine kernels, the
continuation's one-launch reset) the case is pinned to the constant and names the source line.

The expected side of every case was written from choose_step_form (engine_core.hip) and analyze_pattern / pattern_class_ex (capi.hip),
not from a run.

Bars (none is new): 64-bit types 1e-12 on H, V and w, with the oracle's own basis asserted orthogonal to 1e-13 in every full-window
case; 32-bit types at m <= 32 the fixed 2e-5 (w) / 3e-5 (H, V) and the 20 x rule of test_option_form_matches_oracle, beyond m = 32
(where the project has no fixed bar) the 20 x rule alone: the device within 20 x the distance between the oracle run in 32-bit arithmetic
and the fp64 oracle on the same inputs.  Both numbers are printed."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_oracle as ko
from tests import limits
from tests._util import close, relerr
from tests.limits import LIMITS
from tests.option_forms import OPTION_SETS, RESIDENT_SIZES, context_with
from tests.test_gpu_option_forms import _banded, _dense, _grid, _hermitian_part, _random_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


F64, C128, F32, C64 = np.float64, np.complex128, np.float32, np.complex64
TYPES = (F64, C128, F32, C64)
PIPE = frozenset({"pipeline", "overlapped"})
PATCH = PIPE | {"patch"}
WAVE = PIPE | {"wave"}
TWO_KERNEL = frozenset({"two_kernel"})
MODULAR = frozenset({"modular"})

PIPE_CH, LOWSYNC_MAX = LIMITS["PIPE_CH"], LIMITS["LOWSYNC_MAX"]


def _cplx(T):
    return np.dtype(T).kind == "c"


def _is32(T):
    return np.dtype(T).itemsize == (8 if _cplx(T) else 4)


def _T64(T):
    return np.dtype(C128 if _cplx(T) else F64)


def _name(T):
    return np.dtype(T).name


# ------------------------------------------------------------------ operators built from explicit offset lists ------------------
def _diagonals(n, T, offsets, seed, keep=None):
    """i.i.d. normal entries x 0.3 sqrt(5 / k) on the k diagonals `offsets`, the main diagonal shifted by -0.5 (constant or slowly
    varying coefficients per diagonal lose the oracle's orthogonality to 1e-7 .. 1e-3 at these window lengths; these stay at 2e-15).
    keep: {offset: number of leading rows that carry it} for a diagonal that is only partly there"""
    rng = np.random.default_rng([n, seed])
    k = len(offsets)
    rows, cols, vals = [], [], []
    for o in offsets:
        r = np.arange(max(0, -o), min(n, n - o))
        if keep and o in keep:
            r = r[: keep[o]]
        v = rng.standard_normal(len(r)) * 0.3 * math.sqrt(5.0 / k) - (0.5 if o == 0 else 0.0)
        rows.append(r)
        cols.append(r + o)
        vals.append(v * ((1 + 0.25j) if _cplx(T) else 1.0))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A.astype(T)


W8 = LIMITS["PIPE_WMAX"]
# half-bandwidth PIPE_WMAX with PIPE_DIA_MAX diagonals / one diagonal more / PIPE_DIA_MAX diagonals reaching one row further
OFFS_HB8_D8 = (-W8, -3, -1, 0, 1, 2, 5, W8)
OFFS_HB8_D9 = (-W8, -3, -1, 0, 1, 2, 5, 6, W8)
OFFS_HB9_D8 = (-W8 - 1, -3, -1, 0, 1, 2, 5, W8 + 1)
assert len(OFFS_HB8_D8) == LIMITS["PIPE_DIA_MAX"] == len(OFFS_HB9_D8) and len(OFFS_HB8_D9) == LIMITS["PIPE_DIA_MAX"] + 1
# GDIA_MAX distinct offsets reaching over tiles (beyond 512 / 1024 rows), and one more
_FAR = (1, 2, 3, 5, 7, 11, 13, 64, 65, 130, 600, 601, 1100, 1101, 1300)
OFFS_32 = tuple(sorted((0, 17) + _FAR + tuple(-o for o in _FAR)))[: LIMITS["GDIA_MAX"]]
OFFS_33 = tuple(sorted(OFFS_32 + (-17,)))
assert len(set(OFFS_32)) == LIMITS["GDIA_MAX"] == 32 and len(set(OFFS_33)) == LIMITS["GDIA_MAX"] + 1


def _fill_pair_keep(n, over):
    """three full diagonals and five that only the leading rows carry, q entries in all (contiguous rows: the SELL slots stay regular):
    the smallest q that meets analyze_pattern's zero-fill rule nd n <= 1.3 nnz + 1024, or (over) one entry fewer"""
    extra = (-4, -3, -2, 2, 3)
    full = 3 * n - 2
    q = next(q for q in range(0, 5 * n) if limits.fill_ok(8, n, full + q))
    assert q > 5 * 64 and not limits.fill_ok(8, n, full + q - 1)
    q -= 1 if over else 0
    rows_each, rest = divmod(q, 5)
    # (every partly filled diagonal starts at row 4, so that the rows before carry none: same count per row, one ragged row at the end)
    keep = {o: rows_each + (1 if i < rest else 0) for i, o in enumerate(extra)}
    return keep, full + q


def _fill_pair(n, T, over):
    keep, nnz = _fill_pair_keep(n, over)
    rng = np.random.default_rng([n, 88])
    rows, cols, vals = [], [], []
    for o in (-4, -3, -2, -1, 0, 1, 2, 3):
        r = np.arange(max(0, -o), min(n, n - o))
        if o in keep:
            r = np.arange(4, 4 + keep[o])
        v = rng.standard_normal(len(r)) * 0.3 * math.sqrt(5.0 / 8) - (0.5 if o == 0 else 0.0)
        rows.append(r)
        cols.append(r + o)
        vals.append(v * ((1 + 0.25j) if _cplx(T) else 1.0))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    assert A.nnz == nnz and limits.fill_ok(8, n, A.nnz) == (not over)
    return A.astype(T)


def _wave_far(n, T):
    """a grid-like stencil (rows of 200 cells, full diagonals) + one pair of diagonals 99 tiles and a few rows away: with more than 400
    tiles the second clause of the residency rule, (reach / tile + 2) * 4 <= 400, fails too"""
    far = limits.wave_reach_tiles_min() * limits.tile_rows(np.dtype(T).itemsize) + 5
    return _diagonals(n, T, (-far, -200, -1, 0, 1, 200, far), 41)


OPERATORS = {
    "banded": lambda n, T: _banded(n, T, False),
    "banded_herm": lambda n, T: _hermitian_part(_banded(n, T, False).astype(_T64(T)), T),
    "grid5": lambda n, T: _grid(n, T, 5),
    "random_rows": _random_rows,
    "dense": _dense,
    "hb8_d8": lambda n, T: _diagonals(n, T, OFFS_HB8_D8, 51),
    "hb8_d9": lambda n, T: _diagonals(n, T, OFFS_HB8_D9, 52),
    "hb9_d8": lambda n, T: _diagonals(n, T, OFFS_HB9_D8, 53),
    "offsets32": lambda n, T: _diagonals(n, T, OFFS_32, 54),
    "offsets33": lambda n, T: _diagonals(n, T, OFFS_33, 55),
    "fill_under": lambda n, T: _fill_pair(n, T, False),
    "fill_over": lambda n, T: _fill_pair(n, T, True),
    "wave_far": _wave_far,
}


@functools.lru_cache(maxsize=3)
def _operator(opname, Tname, n):
    return OPERATORS[opname](n, np.dtype(Tname))


@functools.lru_cache(maxsize=3)
def _rhs(Tname, n):
    T = np.dtype(Tname)
    rng = np.random.default_rng([n, 7])
    return (rng.standard_normal(n) + (1j * rng.standard_normal(n) if _cplx(T) else 0)).astype(T)


@functools.lru_cache(maxsize=6)
def _oracle(opname, Tname, n, m, iop, herm=False, arith32=False):
    """the oracle's subspace on exactly the values the device has, in 64-bit arithmetic (arith32: in the 32-bit type itself -- the scale
    of the 20 x rule); a full window of a 64-bit type must be orthogonal to rounding, or the 1e-12 bar means nothing"""
    T = np.dtype(Tname)
    A, b = _operator(opname, Tname, n), _rhs(Tname, n)
    if not arith32:
        A, b = A.astype(_T64(T)), b.astype(_T64(T))
    K = ko.arnoldi(A, b, m=m, iop=iop, ishermitian=herm)
    if iop == 0 and not _is32(T):
        V = np.asarray(K.getV())[:, : K.m + 1]
        loss = float(np.max(np.abs(V.conj().T @ V - np.eye(V.shape[1]))))
        assert loss < 1e-13, (opname, Tname, n, m, loss)
    return K


def _bars(T, m, dev, K64, opname, n, iop, herm=False):
    """{which: bar} for H, V, w of one call (module docstring); `dev` is unused for the 64-bit types"""
    if not _is32(T):
        return {"H": 1e-12, "V": 1e-12, "w": 1e-12}, None
    K32 = _oracle(opname, _name(T), n, m, iop, herm, True)
    T64 = _T64(T)
    H64, V64 = np.asarray(K64.getH()), np.asarray(K64.getV())
    rH = float(np.max(np.abs(np.asarray(K32.getH()).astype(T64) - H64)) / np.max(np.abs(H64)))
    rV = float(np.max(np.abs(np.asarray(K32.getV()).astype(T64) - V64)))
    w64 = ko.expv_(np.empty(n, dtype=T64), 0.6, K64)
    w32 = np.asarray(ko.expv_(np.empty(n, dtype=T), 0.6, K32)).astype(T64)
    rw = float(np.linalg.norm(w32 - w64) / np.linalg.norm(w64))
    rule = {"H": 20 * rH + 1e-7, "V": 20 * rV + 1e-7, "w": 20 * rw + 1e-7}
    print("[parity] %-90s H %.3e  V %.3e  w %.3e" % ("  the oracle in %s arithmetic vs the fp64 oracle (m=%d)" % (_name(T), m), rH, rV, rw))
    if m <= 32:
        fixed = {"H": 3e-5, "V": 3e-5, "w": 2e-5}
        return {k: min(fixed[k], rule[k]) for k in fixed}, rule
    return rule, rule


def _deltas(ctx, fn):
    c0 = ctx.counters()
    out = fn()
    c1 = ctx.counters()
    return out, {k: c1[k] - c0[k] for k in c1}


def _launches(ctx, fn):
    """fn() with the per-kernel profile on: {kernel: launches}.  (The profile serialises the single-pass step: never around a case
    whose overlapped form or whose pipelined-Lanczos dispatch -- `!c->prof_on` -- is the subject.)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        got = {k: v["launches"] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    return out, got


def _clean(ctx):
    c = ctx.counters()
    assert c["redo_serial"] == 0 and c["redo_wave_off"] == 0, c


def _check_call(eu, ctx, opname, T, n, m, iop, words, tag, herm=False, op=None, V_too=True):
    """expv (path words, w), arnoldi (counters, H entrywise, V max abs) of one (operator, type, size, m, iop) against the oracle"""
    T = np.dtype(T)
    T64 = _T64(T)
    A, b = _operator(opname, T.name, n), _rhs(T.name, n)
    op = op or eu.MIOperator(A, ctx)
    Ko = _oracle(opname, T.name, n, m, iop, herm)
    bars, _ = _bars(T, m, None, Ko, opname, n, iop, herm)
    w = np.asarray(eu.expv(0.6, op, b, m=m, iop=iop, ishermitian=herm))
    path = frozenset(eu.expv.last_stats["path"])
    print("[path] %-90s %s" % (tag + ": expv", "+".join(sorted(path))))
    assert path == words, "%s: expv ran on %s, the source says %s" % (tag, sorted(path), sorted(words))
    assert w.dtype == T
    close(w.astype(T64), ko.expv_(np.empty(n, dtype=T64), 0.6, Ko), bars["w"], tag + ": expv")
    Ks, d = _deltas(ctx, lambda: eu.arnoldi(op, b, m=m, iop=iop, ishermitian=herm))
    want = {"factorisations": 1, "pipeline": int("pipeline" in words), "overlapped": int("overlapped" in words), "redo_serial": 0,
            "redo_wave_off": 0}
    got = {k: d[k] for k in want}
    print("[counters] %-88s %s" % (tag + ": arnoldi", got))
    assert got == want, "%s: counters %r, expected %r" % (tag, got, want)
    assert Ks.m == Ko.m == m and not Ks.wasbreakdown and not Ko.wasbreakdown
    H = np.asarray(Ks.getH())
    if herm:
        close(H.astype(np.float64), np.real(Ko.getH()), bars["H"], tag + ": H", mat=True)
    else:
        close(H.astype(T64), Ko.getH(), bars["H"], tag + ": H", mat=True)
    if V_too:
        close(np.asarray(Ks.getV()).astype(T64), Ko.getV(), bars["V"], tag + ": V (max abs)", absolute=True)
    return Ks, Ko, bars


# ------------------------------------------------------------------ single-pass window -------------------------------------------
def _single_pass_words(opname, oset, T):
    # choose_step_form: `wstep <= dev::pipe_max_window<T>()` (= PIPE_CH - 1 = 31 for every type), wstep = min(m - 1, iop); the halo
    # form on SELL slots (dia = 0) exists for the real types only; the patch form sets use_ring on top
    if opname == "grid5":
        return PATCH
    return PIPE


SINGLE_PASS = [("banded", "default", T) for T in TYPES] + [("banded", "dia0", T) for T in (F64, F32)] + [("grid5", "patch1", T) for T in TYPES]
# (m, iop, inside): a full window of m - 1 = 31 / 32 columns, an incomplete one of 31 / 32 at m = 40
WINDOWS = [(PIPE_CH, 0, True), (PIPE_CH + 1, 0, False), (40, PIPE_CH - 1, True), (40, PIPE_CH, False)]


@pytest.mark.parametrize("m,iop,inside", WINDOWS, ids=lambda v: str(v))
@pytest.mark.parametrize("opname,oset,T", SINGLE_PASS, ids=lambda v: v if isinstance(v, str) else _name(v))
def test_single_pass_window(eu, opname, oset, T, m, iop, inside):
    """PIPE_CH / pipe_max_window: the single-pass step keeps a window of PIPE_CH - 1 columns in its LDS sums (gs[], the 31 + 1 slots of
    a set).  31 columns run on it (banded diagonal form for all four types, SELL halo for the real ones, grid patch form), 32 run the
    two-kernel step (a grid or a band is not fresh-and-short enough for the wave form at m = 33 / 40: `m <= dev::PIPE_CH`)."""
    assert limits.pipe_max_window(_cplx(T)) == PIPE_CH - 1
    words = _single_pass_words(opname, oset, T) if inside else TWO_KERNEL
    ctx = context_with(eu, OPTION_SETS[oset])
    tag = "window %s/%s %s m=%d iop=%d" % (opname, oset, _name(T), m, iop)
    _check_call(eu, ctx, opname, T, 4100, m, iop, words, tag)
    _clean(ctx)


# ------------------------------------------------------------------ wave form ------------------------------------------------------
@pytest.mark.parametrize("m", [PIPE_CH, PIPE_CH + 1])
@pytest.mark.parametrize("T", [F64, F32], ids=_name)
def test_wave_form_window(eu, T, m):
    """choose_step_form: the wave form takes `m <= dev::PIPE_CH` (its window is the whole run): m = 32 on it, m = 33 on the two-kernel
    step.  A 5-point grid without the patch ordering (general diagonal form)."""
    ctx = context_with(eu, OPTION_SETS["patch0"])
    _check_call(eu, ctx, "grid5", T, 4100, m, 0, WAVE if m <= PIPE_CH else TWO_KERNEL, "wave grid5/patch0 %s m=%d" % (_name(T), m))
    _clean(ctx)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("T", [F64, F32], ids=_name)
def test_wave_form_residency_rule(eu, T, extra):
    """The 400-tile rule (limits.WAVE_RULE_SOURCES): 400 tiles of the element type run the wave form whatever the reach; with one row
    more (401 tiles) and a pair of diagonals 99 tiles away -- (99 + 2) * 4 > 400 -- neither clause holds: two-kernel step."""
    n = limits.WAVE_TILES_MAX * limits.tile_rows(np.dtype(T).itemsize) + extra
    ctx = context_with(eu, {"patch": 0, "reorder": 0})
    info = eu.host_pattern_info(_operator("wave_far", _name(T), n), dtype=T)
    assert info["general_dia_diagonals"] == 7 and info["general_dia_max_offset"] // limits.tile_rows(np.dtype(T).itemsize) == 99, info
    _check_call(eu, ctx, "wave_far", T, n, 8, 0, TWO_KERNEL if extra else WAVE, "wave residency %s n=%d (%d tiles)" % (_name(T), n, 400 + extra))
    _clean(ctx)


# ------------------------------------------------------------------ two-kernel window / modular launches -------------------------
@pytest.mark.parametrize("m,iop,inside", [(LOWSYNC_MAX, 0, True), (LOWSYNC_MAX + 1, 0, False), (70, LOWSYNC_MAX, True), (70, LOWSYNC_MAX + 1, False)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("opname,oset", [("banded", "default"), ("random_rows", "pipeline0")])
@pytest.mark.parametrize("T", [F64, C128, F32], ids=_name)
def test_two_kernel_window(eu, T, opname, oset, m, iop, inside):
    """LOWSYNC_MAX: the two-kernel step solves the window's triangular system in LDS (gs_s[LOWSYNC_MAX (LOWSYNC_MAX - 1) / 2], fused.hip)
    -- choose_step_form: `min(iop, m) <= dev::LOWSYNC_MAX`.  64 columns on it (a band at m = 64 / 70 is past the single-pass window,
    so that is its default form), 65 on the modular launches."""
    ctx = context_with(eu, OPTION_SETS[oset])
    tag = "two-kernel window %s/%s %s m=%d iop=%d" % (opname, oset, _name(T), m, iop)
    _check_call(eu, ctx, opname, T, 4100, m, iop, TWO_KERNEL if inside else MODULAR, tag)
    _clean(ctx)


@pytest.mark.parametrize("m", [LOWSYNC_MAX, LOWSYNC_MAX + 1, 70])
@pytest.mark.parametrize("opname,n", [("dense", 1030), ("banded", 4100)])
@pytest.mark.parametrize("T", [F64, C128], ids=_name)
def test_modular_launches_switch_arithmetic_mid_run(eu, T, opname, n, m):
    """engine_core.hip steps_modular: `lowsync = ortho != MGS && nd >= 2 && nd <= dev::LOWSYNC_MAX` per STEP -- a full window on the
    modular launches uses the low-synchronisation sums up to step 64 and literal MGS from step 65 on, inside one run.  H by column and V
    against the oracle, and against the same call under ortho = "mgs", at the same bar.  The launch counts prove the switch: one dots
    launch per low-synchronisation step (and for step 1, whose window of one column is literal MGS), j of them for an MGS step j."""
    ctx = context_with(eu, OPTION_SETS["pipeline0_fused0"])
    T64 = _T64(T)
    op, b = eu.MIOperator(_operator(opname, _name(T), n), ctx), _rhs(_name(T), n)
    tag = "modular %s %s m=%d" % (opname, _name(T), m)
    Ko = _oracle(opname, _name(T), n, m, 0)
    Ks, got = _launches(ctx, lambda: eu.arnoldi(op, b, m=m, ishermitian=False))
    want_dots = min(m, LOWSYNC_MAX) + sum(range(LOWSYNC_MAX + 1, m + 1))
    print("[counters] %-88s dots %d (expected %d), update %d, fused_a %d" % (tag, got.get("dots", 0), want_dots, got.get("update", 0), got.get("fused_a", 0)))
    assert got.get("dots", 0) == want_dots == got.get("update", 0) and not got.get("fused_a") and not got.get("fused_b"), got
    Km = eu.arnoldi(op, b, m=m, ishermitian=False, ortho="mgs")
    H, Hm, Ho = np.asarray(Ks.getH()).astype(T64), np.asarray(Km.getH()).astype(T64), np.asarray(Ko.getH())
    for j in sorted({0, 1, LOWSYNC_MAX - 2, LOWSYNC_MAX - 1, LOWSYNC_MAX, m - 1} & set(range(m))):      # (columns either side of the switch ...)
        scale = float(np.max(np.abs(Ho)))
        close(H[:, j] / scale, Ho[:, j] / scale, 1e-12, "%s: H column %d vs oracle (entrywise / max|H|)" % (tag, j + 1), absolute=True)
    close(H, Ho, 1e-12, tag + ": H vs oracle", mat=True)                                                # (... and all of them)
    close(np.asarray(Ks.getV()).astype(T64), Ko.getV(), 1e-12, tag + ": V vs oracle (max abs)", absolute=True)
    close(H, Hm, 1e-12, tag + ": H, ortho auto vs mgs", mat=True)
    close(np.asarray(Ks.getV()).astype(T64), np.asarray(Km.getV()).astype(T64), 1e-12, tag + ": V, ortho auto vs mgs (max abs)", absolute=True)
    w = np.asarray(eu.expv(0.6, op, b, m=m, ishermitian=False))
    assert frozenset(eu.expv.last_stats["path"]) == MODULAR, eu.expv.last_stats
    close(w.astype(T64), ko.expv_(np.empty(n, dtype=T64), 0.6, Ko), 1e-12, tag + ": expv")
    _clean(ctx)


# ------------------------------------------------------------------ step number field -----------------------------------------------
@pytest.mark.parametrize("m", [LIMITS["PIPE_MAX_STEPS"] - 2, LIMITS["PIPE_MAX_STEPS"] - 1])
@pytest.mark.parametrize("T", [F64, C128], ids=_name)
def test_step_number_field(eu, T, m):
    """PIPE_MAX_STEPS: the step number travels in 11 bits of the step flag (flag = seq << 12 | stop << 11 | step); choose_step_form:
    `m + 2 <= dev::PIPE_MAX_STEPS` (m steps, the closing pass, one spare).  m = 1998 on the single-pass step, 1999 on the two-kernel
    step.  iop = 3: a one-rounding perturbation of b moves this H by 1.4e-15 and V by 3.8e-15 (Lanczos at that length moves by 0.16).
    expv! is evaluated once per case, inside the whole-call expv that also reports the path: the library's host exponential of a
    1998 x 1998 Hessenberg matrix is what this case costs (measured: 3 s for Float64, 14 .. 24 s for ComplexF64).  Its reference is
    the definition on the oracle's subspace, beta V_m exp(t H_m) e_1 with scipy's exponential -- equal to the oracle's own expv! to
    4e-16 here, whose pure-Python exponential takes 8 s at this size."""
    import scipy.linalg as sl
    n, iop = 4100, 3
    T64 = _T64(T)
    ctx = context_with(eu, OPTION_SETS["default"])
    words = PIPE if m + 2 <= LIMITS["PIPE_MAX_STEPS"] else TWO_KERNEL
    tag = "step field banded %s m=%d iop=3" % (_name(T), m)
    op, b = eu.MIOperator(_operator("banded", _name(T), n), ctx), _rhs(_name(T), n)
    Ko = _oracle("banded", _name(T), n, m, iop)
    w = np.asarray(eu.expv(0.6, op, b, m=m, iop=iop, ishermitian=False))
    path = frozenset(eu.expv.last_stats["path"])
    print("[path] %-90s %s" % (tag + ": expv", "+".join(sorted(path))))
    assert path == words, "%s: expv ran on %s, the source says %s" % (tag, sorted(path), sorted(words))
    Ho, Vo = np.asarray(Ko.getH()), np.asarray(Ko.getV())
    close(w.astype(T64), Ko.beta * (Vo[:, :m] @ sl.expm(0.6 * Ho[:m, :m])[:, 0]), 1e-12, tag + ": expv! (whole call)")
    Ks, d = _deltas(ctx, lambda: eu.arnoldi(op, b, m=m, iop=iop, ishermitian=False))
    print("[counters] %-88s %s" % (tag + ": arnoldi", d))
    assert (d["factorisations"], d["pipeline"], d["overlapped"]) == (1, int("pipeline" in words), int("overlapped" in words)), d
    assert Ks.m == Ko.m == m and not Ks.wasbreakdown
    close(np.asarray(Ks.getH()).astype(T64), Ho, 1e-12, tag + ": H", mat=True)
    close(np.asarray(Ks.getV()).astype(T64), Vo, 1e-12, tag + ": V (max abs)", absolute=True)
    _clean(ctx)


# ------------------------------------------------------------------ augmented operator (kiops) ---------------------------------------
@functools.lru_cache(maxsize=2)
def _kiops_inputs(cplx, ncols):
    n = 4100
    rng = np.random.default_rng([31, ncols])
    A = _banded(n, C128 if cplx else F64, False)
    u = rng.standard_normal((n, ncols)) + (1j * rng.standard_normal((n, ncols)) if cplx else 0)
    # (column j scaled by 1 / j!: a one-rounding perturbation of u then moves the result by 3e-16 with identical statistics)
    return A, np.asfortranarray(u * np.array([1.0 / math.factorial(j) for j in range(ncols)]) * 30)


@functools.lru_cache(maxsize=4)
def _kiops_oracle(cplx, ncols, iop):
    A, u = _kiops_inputs(cplx, ncols)
    return ko.kiops(2.0, A, u, allow_complex=cplx, ishermitian=False, iop=iop, tol=1e-10)


@pytest.mark.parametrize("iop", [7, 8])
@pytest.mark.parametrize("p", [LIMITS["PIPE_AUG_MAX"], LIMITS["PIPE_AUG_MAX"] + 1])
@pytest.mark.parametrize("cplx", [False, True], ids=["float64", "complex128"])
def test_kiops_augmentation_width(eu, cplx, p, iop):
    """PIPE_AUG_MAX / FUSED_AUG_MAX: the p extra rows of kiops' augmented operator live in `ut[PIPE_AUG_MAX]` of the single-pass step
    and in the first kernel of the two-kernel step.  choose_step_form: single-pass `p <= PIPE_AUG_MAX && min(m, iop) <= 7`, two-kernel
    `p <= FUSED_AUG_MAX`, else the modular launches.  u with p + 1 columns: p = 8, iop = 7 every factorisation on the single-pass
    step; p = 8, iop = 8 the two-kernel step; p = 9 the modular launches (+ the `aug` kernel)."""
    A, u = _kiops_inputs(cplx, p + 1)
    wo, so = _kiops_oracle(cplx, p + 1, iop)
    ctx = context_with(eu, OPTION_SETS["default"])
    op = eu.MIOperator(A, ctx)
    tag = "kiops %s p=%d iop=%d" % ("complex128" if cplx else "float64", p, iop)
    run = lambda: eu.kiops(2.0, op, u, allow_complex=cplx, ishermitian=False, iop=iop, tol=1e-10)
    single_pass = p <= LIMITS["PIPE_AUG_MAX"] and iop <= 7
    if single_pass:
        (w, st), d = _deltas(ctx, run)
        print("[counters] %-88s %s" % (tag, d))
        assert d["pipeline"] == d["factorisations"] >= 2 and d["overlapped"] == d["factorisations"], d
    else:
        ((w, st), got), d = _deltas(ctx, lambda: _launches(ctx, run))
        print("[counters] %-88s %s  launches %s" % (tag, d, got))
        assert d["pipeline"] == 0 and d["factorisations"] >= 2, d
        # (engine_core.hip: update2 of the two-kernel step is profiled as fused_b, the update of the modular launches as update)
        if p <= LIMITS["FUSED_AUG_MAX"]:
            assert got.get("fused_a", 0) > 0 and got.get("fused_b", 0) > 0 and not got.get("update") and not got.get("aug"), got
        else:
            assert got.get("dots", 0) > 0 and got.get("update", 0) > 0 and got.get("aug", 0) > 0 and not got.get("fused_b"), got
    assert tuple(st) == tuple(so), (tag, st, so)
    close(w, wo, 1e-12, tag + " vs oracle")
    _clean(ctx)


# ------------------------------------------------------------------ phiv_timestep's update --------------------------------------------
@functools.lru_cache(maxsize=2)
def _timestep_inputs(ncols):
    n = 4100
    rng = np.random.default_rng([32, ncols])
    A = ((_banded(n, F64, False) - 1.6 * sp.eye(n)) * 4.0).tocsr()      # (decaying and stiff enough for several sub-steps)
    A.sort_indices()
    B = rng.standard_normal((n, ncols)) * np.array([1.0 / math.factorial(j) for j in range(ncols)])
    return A, np.asfortranarray(B)


TS = (8.0, 20.0)


@functools.lru_cache(maxsize=4)
def _timestep_oracle(ncols, m, adaptive):
    A, B = _timestep_inputs(ncols)
    so = {}
    U = ko.phiv_timestep(np.array(TS), A, B, adaptive=adaptive, tol=1e-10, m=m, stats=so)
    return U, so


_CBV = LIMITS["COEF_BY_VALUE_MAX"]


@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "fixed"])
@pytest.mark.parametrize("ncols,m", [(7, 20), (8, 20), (3, _CBV - 2), (3, _CBV - 1), (3, _CBV), (3, _CBV + 1)])
def test_phiv_timestep_update_forms(eu, ncols, m, adaptive):
    """engine_drivers.hip, u_update: `p <= 6 && mext <= dev::COEF_BY_VALUE_MAX` -- the sub-step's update as ONE combine with a tail of
    at most six terms (LcTerms::in[6], apply_lincomb's six terms) and the coefficients by value (CoefVec::c[COEF_BY_VALUE_MAX]), else
    the column followed by a lincomb launch.  B with 7 / 8 columns (p = 6 / 7); at least three sub-steps.
    The coefficient column: the cases m + p = 64 / 65 were written expecting m + p coefficients.  Reading the source says otherwise --
    `mext` comes from phiv_coefficients, mext = m + (correct ? 1 : 0), the SUBSPACE's column count, not the augmented one -- and the
    first run agreed: m = 62 and 63 with p = 2 both take the one-combine form (no lincomb launch).  They stay; m = 64 / 65 are the two
    sides of the limit as the source has it."""
    p = ncols - 1
    A, B = _timestep_inputs(ncols)
    Uo, so = _timestep_oracle(ncols, m, adaptive)
    assert so["num_timesteps"] >= 3, so
    ctx = context_with(eu, OPTION_SETS["default"])
    op = eu.MIOperator(A, ctx)
    st = {}
    tag = "phiv_timestep p=%d m=%d %s" % (p, m, "adaptive" if adaptive else "fixed")
    U, got = _launches(ctx, lambda: np.asarray(eu.phiv_timestep(np.array(TS), op, B, adaptive=adaptive, tol=1e-10, m=m, stats=st)))
    print("[counters] %-88s sub-steps %d, m %d, lincomb launches %d" % (tag, st["num_timesteps"], st["m"], got.get("lincomb", 0)))
    assert (st["num_timesteps"], st["matvecs"], st["m"]) == (so["num_timesteps"], so["matvecs"], so["m"]), (st, so)
    close(U, Uo, 1e-12, tag + " vs oracle")
    if p > 6 or (not adaptive and m > _CBV):
        assert got.get("lincomb", 0) > 0, got
    elif not adaptive or m == 20:      # (an adaptive run changes m between sub-steps: certain only where it starts far from the limit)
        assert got.get("lincomb", 0) == 0, got
    _clean(ctx)


# ------------------------------------------------------------------ combine kernels ----------------------------------------------------
_MEXT_MAX = LIMITS["COEF_MAT_MAX"] // LIMITS["COEF_MAT_COLS"]      # rows of a COEF_MAT_COLS-column matrix that still travels by value


def _bar_w32(m, r):
    """the 32-bit bar of a result vector / matrix whose distance between the two oracles is r (module docstring)"""
    return min(2e-5, 20 * r + 1e-7) if m <= 32 else 20 * r + 1e-7


@pytest.mark.parametrize("T,oset", [(T, "default") for T in TYPES] + [(F64, "reorder2")], ids=lambda v: v if isinstance(v, str) else _name(v))
def test_combine_kernels_at_their_argument_sizes(eu, T, oset):
    """engine_core.hip combine_host_coef / combine_launch: `by_value = ncols == 1 && mcols <= COEF_BY_VALUE_MAX` (combine1, CoefVec::c[64];
    expv! passes mcols = m: m = 64 / 65), `ncols <= COEF_MAT_COLS && mc * ncols <= COEF_MAT_MAX` (combine_v, CoefMat::c[192]; phiv! passes
    ncols = k + 1 and mc = m + correct: k + 1 = 6 / 7 at m = 20, and k + 1 = 6 with m + 1 = 32 / 33), else the coefficients through device
    memory (combine).  Nothing observable separates the three kernels: the cases are pinned to the constants.  Float64 once more
    through a reordered operator (random rows, reorder = 2): the un-permuting store fused into the kernel exists on the by-value side."""
    opname, n = ("random_rows", 4100) if oset == "reorder2" else ("banded", 4100)
    ctx = context_with(eu, OPTION_SETS[oset])
    T64 = _T64(T)
    A, b = _operator(opname, _name(T), n), _rhs(_name(T), n)
    op = eu.MIOperator(A, ctx)
    if oset == "reorder2":
        print("[path] %-90s %s" % ("combine: reorder_info", dict(op.reorder_info).get("reordered")))
    for m in (_CBV, _CBV + 1):
        Ko = _oracle(opname, _name(T), n, m, 0)
        K32 = _oracle(opname, _name(T), n, m, 0, False, True) if _is32(T) else None
        Ks = eu.arnoldi(op, b, m=m, ishermitian=False)
        for t in (0.6, 0.3 - 0.4j):
            Tw = np.result_type(T, np.complex64) if isinstance(t, complex) else T
            w = np.asarray(eu.expv_(np.empty(n, dtype=Tw), t, Ks))
            wo = ko.expv_(np.empty(n, dtype=np.complex128), t, Ko)
            bar = 1e-12
            if K32 is not None:
                r = relerr(np.asarray(ko.expv_(np.empty(n, dtype=Tw), t, K32)).astype(np.complex128), wo)
                bar = _bar_w32(m, r)
                print("[parity] %-90s w %.3e" % ("  the oracle in %s arithmetic vs the fp64 oracle (m=%d, t=%s)" % (_name(T), m, t), r))
            close(w.astype(np.complex128), wo, bar, "combine %s %s: expv! with %d coefficients, t=%s" % (oset, _name(T), m, t))
    for m, k, correct in ((20, LIMITS["COEF_MAT_COLS"] - 1, False), (20, LIMITS["COEF_MAT_COLS"], False),
                          (_MEXT_MAX - 1, LIMITS["COEF_MAT_COLS"] - 1, True), (_MEXT_MAX, LIMITS["COEF_MAT_COLS"] - 1, True),
                          (_MEXT_MAX, LIMITS["COEF_MAT_COLS"] - 1, False), (_MEXT_MAX + 1, LIMITS["COEF_MAT_COLS"] - 1, False)):
        Ko = _oracle(opname, _name(T), n, m, 0)
        Ks = eu.arnoldi(op, b, m=m, ishermitian=False)
        W = np.asarray(eu.phiv_(np.empty((n, k + 1), dtype=T, order="F"), 0.5, Ks, k, correct=correct))
        Wo = ko.phiv_(np.empty((n, k + 1), dtype=T64, order="F"), 0.5, Ko, k, correct=correct)
        bar = 1e-12
        if _is32(T):
            K32 = _oracle(opname, _name(T), n, m, 0, False, True)
            r = relerr(np.asarray(ko.phiv_(np.empty((n, k + 1), dtype=T, order="F"), 0.5, K32, k, correct=correct)).astype(T64), Wo)
            bar = _bar_w32(m, r)
            print("[parity] %-90s W %.3e" % ("  the oracle in %s arithmetic vs the fp64 oracle (m=%d, k=%d)" % (_name(T), m, k), r))
        close(W.astype(T64), Wo, bar, "combine %s %s: phiv! %d x %d coefficients (m=%d, correct=%s)" % (oset, _name(T), m + int(correct), k + 1, m, correct))
    _clean(ctx)


# ------------------------------------------------------------------ continuation ---------------------------------------------------------
@pytest.mark.parametrize("j", [LIMITS["CONT_SCALES_MAX"] - 1, LIMITS["CONT_SCALES_MAX"], LIMITS["CONT_SCALES_MAX"] + 1])
def test_continuation_reset_at_the_scale_limit(eu, j):
    """engine_core.hip reset_device_state: `use_pipe && !fresh && jstart <= dev::CONT_SCALES_MAX` -- a continued single-pass
    factorisation resets state, tickets and the stored columns' scales in ONE launch whose arguments hold CONT_SCALES_MAX scales;
    from column 161 on the copies and memsets of steps_single_pass do it.  Nothing observable separates the two: pinned to the constant.
    arnoldi!(...; init = j) up to m = 170 against a from-scratch run (1e-13) and the oracle (1e-12)."""
    n, m, iop = 4100, 170, 3
    ctx = context_with(eu, OPTION_SETS["default"])
    op, b = eu.MIOperator(_operator("banded", "float64", n), ctx), _rhs("float64", n)
    Ks = eu.KrylovSubspace(F64, F64, n, m, 0, ctx)
    eu.arnoldi_(Ks, op, b, m=j, iop=iop, ishermitian=False)
    _, d = _deltas(ctx, lambda: eu.arnoldi_(Ks, op, b, m=m, iop=iop, init=j, ishermitian=False))
    print("[counters] %-88s %s" % ("continuation %d -> %d" % (j, m), d))
    assert d["pipeline"] == 1 and d["krylov_steps"] == m - j + 1 and d["redo_serial"] == 0, d
    Kf = eu.KrylovSubspace(F64, F64, n, m, 0, ctx)
    eu.arnoldi_(Kf, op, b, m=m, iop=iop, ishermitian=False)
    close(Ks.getH(), Kf.getH(), 1e-13, "continuation %d -> %d (iop 3): H vs from scratch" % (j, m), mat=True)
    close(Ks.getV(), Kf.getV(), 1e-13, "continuation %d -> %d (iop 3): V vs from scratch (max abs)" % (j, m), absolute=True)
    Ko = _oracle("banded", "float64", n, m, iop)
    close(Ks.getH(), Ko.getH(), 1e-12, "continuation %d -> %d (iop 3): H vs oracle" % (j, m), mat=True)
    close(Ks.getV(), Ko.getV(), 1e-12, "continuation %d -> %d (iop 3): V vs oracle (max abs)" % (j, m), absolute=True)
    _clean(ctx)


# ------------------------------------------------------------------ pipelined Lanczos -------------------------------------------------------
@pytest.mark.parametrize("n,m", [(4100, LIMITS["PL_MAX_M"]), (4100, LIMITS["PL_MAX_M"] + 1), (2 * W8 * 3, 12), (2 * W8 * 3 - 1, 12)])
def test_pipelined_lanczos_limits(eu, n, m):
    """engine_core.hip lanczos_pipelined_applies: `m <= dev::PL_MAX_M` (al[PL_MAX_M + 3], be[PL_MAX_M + 3] in LDS) and
    `ks.n >= 2 * dev::PIPE_WMAX * 3`.  The Hermitian part of the banded operator (the oracle's Lanczos basis on it stays orthogonal to
    1.05e-14 at m = 129); bars of test_pipelined_lanczos_opt_in_mode on the pipelined side, the default path's on the other.  (No
    per-kernel profile here: `!c->prof_on` is part of the dispatch.)"""
    inside = m <= LIMITS["PL_MAX_M"] and n >= 2 * W8 * 3
    ctx = context_with(eu, OPTION_SETS["default"])
    A, b = _operator("banded_herm", "float64", n), _rhs("float64", n)
    op = eu.MIOperator(A, ctx)
    tag = "pipelined Lanczos n=%d m=%d" % (n, m)
    wc = np.asarray(eu.expv(0.7, op, b, m=m, ishermitian=True, ortho="pipelined"))
    path = frozenset(eu.expv.last_stats["path"])
    print("[path] %-90s %s" % (tag + ": expv", "+".join(sorted(path))))
    assert ("pipelined_lanczos" in path) == inside, (tag, sorted(path))
    Ko = ko.KrylovSubspace(F64, F64, n, m)
    ko.lanczos_(Ko, A, b, m=m)
    Vo = np.asarray(Ko.getV())[:, : m + 1]
    assert float(np.max(np.abs(Vo.T @ Vo - np.eye(m + 1)))) < 1e-13
    Ks = eu.KrylovSubspace(F64, F64, n, m, 0, ctx)
    eu.lanczos_(Ks, op, b, m=m, ortho="pipelined")
    assert Ks.m == Ko.m == m and not Ks.wasbreakdown
    assert abs(Ks.beta - Ko.beta) <= 1e-13 * Ko.beta
    bar = 1e-11 if inside else 1e-12
    close(np.asarray(Ks.getH()), Ko.getH(), bar, tag + ": H vs the reference recurrence", mat=True)
    wo = ko.expv_(np.empty(n), 0.7, Ko)
    close(np.asarray(eu.expv_(np.empty(n), 0.7, Ks)), wo, bar, tag + ": expv! vs the reference recurrence")
    close(wc, wo, bar, tag + ": whole-call expv vs the reference recurrence")
    V = np.asarray(Ks.getV())[:, :m]
    eo = float(np.abs(V.T @ V - np.eye(m)).max())
    print("[parity] %-90s err %.3e  (bar %.1e)" % (tag + ": basis orthonormal", eo, 1e-9))
    assert eo < 1e-9
    _clean(ctx)


# ------------------------------------------------------------------ resident kernel ------------------------------------------------------------
@pytest.mark.parametrize("m", [PIPE_CH - 1, PIPE_CH, PIPE_CH + 1])
def test_resident_kernel_window(eu, m):
    """engine_core.hip steps_single_pass / pipe.hip pipe_resident: `m + (closing ? 1 : 0) <= dev::PIPE_CH`.  Read from the source: the
    whole-call expv asks for no closing pass (Ks::skip_tail), so IT runs the resident kernel up to m = PIPE_CH = 32 -- the `resident`
    word is present at m = 31 and 32, absent at 33 (two-kernel step); arnoldi! wants v_{m+1}, and `closing` needs min(m, iop) <= 31: it
    runs the resident kernel with its closing pass at m + 1 = PIPE_CH and the step-wise form at m = 32 (no path word there: compared
    with the oracle on both sides)."""
    n = RESIDENT_SIZES[0]
    ctx = context_with(eu, OPTION_SETS["resident"])
    words = (PIPE | {"resident"}) if m <= PIPE_CH else TWO_KERNEL
    _check_call(eu, ctx, "banded", F64, n, m, 0, words, "resident banded float64 n=%d m=%d" % (n, m))
    _clean(ctx)


# ------------------------------------------------------------------ expv_batch refusals --------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _batch_inputs(n, nprob=2):
    rng = np.random.default_rng(n + 16)
    A0 = _banded(n, F64, False)
    A0.sort_indices()
    vals = np.stack([A0.data * s for s in (1 + 0.1 * rng.random(nprob))])
    B = np.asfortranarray(rng.standard_normal((n, nprob)))
    return A0, vals, B


def _batch_matches_oracle(eu, ctx, n, m, iop, tag):
    A0, vals, B = _batch_inputs(n)
    W, mu = eu.expv_batch(0.8, A0, vals, B, m=m, iop=iop, ctx=ctx, return_m=True)
    assert all(int(x) == m for x in mu)
    for p in range(vals.shape[0]):
        Ap = A0.copy()
        Ap.data = vals[p].copy()
        close(np.asarray(W)[:, p], ko.expv(0.8, Ap, B[:, p], m=m, iop=iop, ishermitian=False), 1e-12, "%s: problem %d vs the oracle's expv" % (tag, p))


@pytest.mark.parametrize("what", ["window", "steps", "rows"])
def test_expv_batch_refusals(eu, what):
    """engine_batch.hip: `min(iop, m) > dev::LOWSYNC_MAX` and `m > dev::LOWSYNC_MAX * 2` are refused with Unsupported, and so is
    `ntiles > dev::MAX_GRID` on the batched single-pass step (its partial sums are MAX_GRID * 64 per problem).  The last valid value runs
    and matches the oracle; after each refusal the same context gives the oracle's answer on a valid call."""
    ctx = context_with(eu, OPTION_SETS["default"])
    if what == "window":
        good, bad, n = dict(m=LOWSYNC_MAX, iop=0), dict(m=LOWSYNC_MAX + 1, iop=0), 4100
    elif what == "steps":
        good, bad, n = dict(m=2 * LOWSYNC_MAX, iop=3), dict(m=2 * LOWSYNC_MAX + 1, iop=3), 4100
    else:
        good, bad, n = None, dict(m=8, iop=0), (LIMITS["MAX_GRID"] + 1) * limits.tile_rows(8)
    if good:
        _batch_matches_oracle(eu, ctx, n, good["m"], good["iop"], "expv_batch m=%d iop=%d (last valid)" % (good["m"], good["iop"]))
    A0, vals, B = _batch_inputs(n)
    with pytest.raises(eu.ExpvMIError) as e:
        eu.expv_batch(0.8, A0, vals, B, ctx=ctx, **bad)
    print("[state] expv_batch n=%d %r: %s" % (n, bad, e.value))
    assert e.value.code == 5, e.value                       # EXPV_MI_UNSUPPORTED
    _batch_matches_oracle(eu, ctx, 4100, 16, 0, "expv_batch after the refusal (%s) on the same context" % what)
    if what == "rows":      # ... and MAX_GRID tiles exactly still run
        n = LIMITS["MAX_GRID"] * limits.tile_rows(8)
        _batch_matches_oracle(eu, ctx, n, 8, 0, "expv_batch n=%d (MAX_GRID tiles)" % n)
    _clean(ctx)


# ------------------------------------------------------------------ pattern analysis --------------------------------------------------------------
def _pattern_words(opname, T):
    """capi.hip analyze_pattern -> pattern_class_ex -> choose_step_form, for contexts with patch = 0 and reorder = 0 at m = 20:
       pipe_dia  = fill_ok && bandwidth <= PIPE_WMAX && nd <= PIPE_DIA_MAX     -> halo form on the diagonal form, every type
       bandwidth <= PIPE_WMAX without it                                        -> halo form on SELL slots, real types; complex: two-kernel
       general_dia (<= GDIA_MAX offsets, fill_ok) or bounded tile reach          -> wave form, real types (<= 400 tiles here); complex: two-kernel"""
    real = not _cplx(T)
    if opname in ("hb8_d8", "fill_under"):
        return PIPE
    if opname in ("hb8_d9", "fill_over"):
        return PIPE if real else TWO_KERNEL
    return WAVE if real else TWO_KERNEL      # hb9_d8, offsets32 (general diagonal form), offsets33 (SELL slots, tile reach)


def _pattern_info_expected(opname):
    """(pipeline_dia_diagonals, general_dia_diagonals) of host_pattern_info: which diagonal form the analysis gives"""
    return {"hb8_d8": (8, 0), "hb8_d9": (0, 9), "hb9_d8": (0, 8), "offsets32": (0, 32), "offsets33": (0, 0), "fill_under": (8, 0),
            "fill_over": (0, 0)}[opname]


@pytest.mark.parametrize("n", [4100, 70_001])
@pytest.mark.parametrize("T", TYPES, ids=_name)
@pytest.mark.parametrize("opname", ["hb8_d8", "hb8_d9", "hb9_d8", "offsets32", "offsets33", "fill_under", "fill_over"])
def test_pattern_analysis_limits(eu, opname, T, n):
    """PIPE_WMAX, PIPE_DIA_MAX, GDIA_MAX and the zero-fill rule of capi.hip analyze_pattern (doff[PIPE_DIA_MAX], the halo rows, the
    general form's offset array): half-bandwidth 8 with 8 / 9 diagonals, half-bandwidth 9 with 8, 32 / 33 distinct offsets reaching over
    tiles, and a pair whose zero fill lies just under / one entry over nd n <= 1.3 nnz + 1024.  What the analysis decides is asserted on
    host_pattern_info; the step form it leads to on the path words (the real types of the fill pair run the halo form either way -- on
    the diagonal form or on SELL slots: the analysis result is what separates them)."""
    A = _operator(opname, _name(T), n)
    info = eu.host_pattern_info(A, dtype=T)
    print("[path] %-90s %s" % ("pattern %s %s n=%d" % (opname, _name(T), n), {k: info[k] for k in ("bandwidth", "pipeline_dia_diagonals", "general_dia_diagonals", "sell_wave_reach", "sell_cut")}))
    assert (info["pipeline_dia_diagonals"], info["general_dia_diagonals"]) == _pattern_info_expected(opname) and info["sell_cut"] == 0, info
    ctx = context_with(eu, {"patch": 0, "reorder": 0})
    _check_call(eu, ctx, opname, T, n, 20, 0, _pattern_words(opname, T), "pattern %s %s n=%d m=20" % (opname, _name(T), n))
    _clean(ctx)


# ------------------------------------------------------------------ grid sizes -----------------------------------------------------------------------
_GROUP, _MAXG = LIMITS["GROUP_SIZE"], LIMITS["MAX_GRID"]
# workgroups: 64 / 65 (the one-group reduction), 128 / 129 (two step grids no larger than the CU count: no residency gate),
# MAX_GRID / MAX_GRID + 1 and a ragged tile more (the grid-stride branch of every `if (g > MAX_GRID) g = MAX_GRID` launch)
GRID_TILES = [(_GROUP, 0), (_GROUP, 1), (2 * _GROUP, 0), (2 * _GROUP, 1), (_MAXG, 0), (_MAXG + 1, 1)]


def _grid_words(form, T, n):
    if form == "random_rows":
        # five entries anywhere in the row: no diagonal form, the tile reach is ~ n; the real types run the wave form on SELL slots
        # while ntiles <= 400 (choose_step_form, `wave_sell`), the two-kernel step beyond; the complex types have no wave form
        tiles = -(-n // limits.tile_rows(np.dtype(T).itemsize))
        return WAVE if (not _cplx(T) and tiles <= limits.WAVE_TILES_MAX) else TWO_KERNEL
    return {"default": PIPE, "pipeline0": TWO_KERNEL, "pipeline0_fused0": MODULAR}[form]


@pytest.mark.parametrize("tiles,extra", GRID_TILES, ids=lambda v: str(v))
@pytest.mark.parametrize("T", [F64, C128], ids=_name)
def test_grid_sizes(eu, T, tiles, extra):
    """GROUP_SIZE, MAX_GROUPS, MAX_GRID (kernels.hip, fused.hip, pipe.hip grid sizing; the partial-sum arrays `part` / `gpart`): row
    counts of exactly 64, 128 and 2048 tiles of the element type, one row more, and 2049 tiles + 1 row, on the single-pass step, the
    two-kernel step, the modular launches, and SELL slots with scattered columns.  m = 8 keeps the oracle at seconds."""
    n = tiles * limits.tile_rows(np.dtype(T).itemsize) + extra
    for form in ("default", "pipeline0", "pipeline0_fused0", "random_rows"):
        opname = "random_rows" if form == "random_rows" else "banded"
        ctx = context_with(eu, {"reorder": 0} if form == "random_rows" else OPTION_SETS[form])
        _check_call(eu, ctx, opname, T, n, 8, 0, _grid_words(form, T, n), "grid %s %s n=%d (%d tiles + %d)" % (form, _name(T), n, tiles, extra))
        _clean(ctx)
