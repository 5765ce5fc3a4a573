"""The compile-time capacity limits of the engine, read from the source; no device work here.

The engine picks a Krylov step form, a combine kernel and a reduction shape by comparing a call against the `constexpr int` constants of
csrc/kernels.h, and every one of them also sizes something fixed on the device (an LDS array, an array inside the kernel arguments, a
bit field).  tests/test_gpu_limits.py runs one call on each side of each limit; its boundary values come from LIMITS, so a changed
constant moves the cases with it -- and tests/test_limits_cpu.py fails when a relation the hand-built inputs rely on stops holding."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "exponentialutilities.jl_amd", "csrc")

# every constant the table of DESIGN.md section 5 ("limits") names
NAMES = ("BLOCK", "GROUP_SIZE", "MAX_GROUPS", "MAX_GRID", "LOWSYNC_MAX", "CONT_SCALES_MAX", "FUSED_AUG_MAX", "GDIA_MAX", "PIPE_CH",
         "PIPE_CH_CPLX", "PIPE_WMAX", "PIPE_DIA_MAX", "PIPE_AUG_MAX", "PIPE_MAX_STEPS", "PL_MAX_M", "COEF_BY_VALUE_MAX", "COEF_MAT_MAX",
         "COEF_MAT_COLS")

_DECL = re.compile(r"constexpr\s+int\s+([^;]+);")
_ITEM = re.compile(r"^\s*([A-Za-z_]\w*)\s*=\s*(.+?)\s*$")
_EXPR = re.compile(r"^[\w\s*+\-()/]+$")


def parse_constants(text):
    """{name: value} of every `constexpr int NAME = value[, NAME2 = value2];` of a header; a value is an integer or an arithmetic
    expression over constants declared before it (MAX_GRID = GROUP_SIZE * MAX_GROUPS)"""
    out = {}
    for decl in _DECL.findall(text):
        for item in decl.split(","):
            m = _ITEM.match(item)
            if not m or not _EXPR.match(m.group(2)):
                continue
            try:
                out[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(out)))
            except Exception:      # (an expression over something that is no integer constant of this header)
                continue
    return out


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def load_limits():
    found = parse_constants(_read("kernels.h"))
    return {k: found[k] for k in NAMES if k in found}


LIMITS = load_limits()

# The residency rule of the wave form is a literal, in two places that must agree:
#   engine_core.hip, choose_step_form:  `(ntiles_w <= 400 || (reach_rows / trw + 2) * 4 <= 400)`
#   capi.hip, pattern_class_ex:         `if (ntiles <= 400 || (reach / trw + 2) * 4 <= 400) return {2, reach, wave_dia};`
WAVE_TILES_MAX = 400
WAVE_RULE_SOURCES = (("engine_core.hip", "ntiles_w <= 400 || (reach_rows / trw + 2) * 4 <= 400"),
                     ("capi.hip", "ntiles <= 400 || (reach / trw + 2) * 4 <= 400"))
# ... and the zero-fill rule of the diagonal forms (capi.hip, analyze_pattern): `nd * n <= 1.3 * nnz + 1024.0`
FILL_RULE_SOURCE = ("capi.hip", "(double)nd * (double)n <= 1.3 * (double)nnz + 1024.0")
# the pipelined Lanczos recurrence needs n >= 2 * PIPE_WMAX * 3 rows (engine_core.hip, lanczos_pipelined_applies)
PL_MIN_ROWS_SOURCE = ("engine_core.hip", "ks.n >= 2 * dev::PIPE_WMAX * 3")


def wave_reach_tiles_min():
    """smallest reach, in whole tiles, at which the second clause of the residency rule fails too: (reach / trw + 2) * 4 > 400"""
    return WAVE_TILES_MAX // 4 - 2 + 1


def source_has(where):
    fname, needle = where
    return needle in _read(fname)


def tile_rows(dtype_itemsize):
    """rows of a tile of the single-pass step: BLOCK lanes x one 16-byte pack"""
    return (16 // dtype_itemsize) * LIMITS["BLOCK"]


def fill_ok(nd, n, nnz):
    """analyze_pattern's zero-fill rule, in the same floating-point expression"""
    return nd > 0 and float(nd) * float(n) <= 1.3 * float(nnz) + 1024.0


def pipe_max_window(is_complex):
    """kernels.h, pipe_max_window<T>(): the longest update window of the single-pass step"""
    return (LIMITS["PIPE_CH_CPLX"] if is_complex else LIMITS["PIPE_CH"]) - 1
