"""tests/limits.py finds every capacity constant in the source, and the relations between them that the hand-built inputs of
tests/test_gpu_limits.py rely on still hold.  A changed constant fails HERE, loudly, instead of moving a GPU case off its boundary."""
import os

from tests import limits
from tests.limits import LIMITS


def test_every_constant_is_found_in_the_source():
    assert set(LIMITS) == set(limits.NAMES), sorted(set(limits.NAMES) - set(LIMITS))
    assert all(isinstance(v, int) and v > 0 for v in LIMITS.values()), LIMITS
    # the parser itself: several declarations in one statement, an expression over earlier constants, things that are no integers
    got = limits.parse_constants("constexpr int A = 4;  // four\nconstexpr int B = 192, C = 6;\nconstexpr int D = A * C;\n"
                                 "constexpr int E = 1 << 30, F = 7;\nconstexpr uint32_t G = 0xfu;\nstatic constexpr int H = 16 / sizeof(T);")
    assert got == {"A": 4, "B": 192, "C": 6, "D": 24, "F": 7}, got


def test_literal_rules_are_where_limits_py_says_they_are():
    for where in limits.WAVE_RULE_SOURCES + (limits.FILL_RULE_SOURCE, limits.PL_MIN_ROWS_SOURCE):
        assert limits.source_has(where), "%s no longer contains `%s`: restate the rule in tests/limits.py" % where
    assert limits.wave_reach_tiles_min() == 99          # (99 / 1 + 2) * 4 = 404 > 400 >= (98 + 2) * 4


def test_relations_the_boundary_cases_rely_on():
    L = LIMITS
    # grid sizing: MAX_GRID workgroups reduce in MAX_GROUPS groups of GROUP_SIZE; the tickets of device_types.h are sized by the same number
    assert L["MAX_GRID"] == L["GROUP_SIZE"] * L["MAX_GROUPS"] and L["GROUP_SIZE"] == 64 and L["BLOCK"] == 256
    with open(os.path.join(limits.CSRC, "device_types.h")) as f:
        assert limits.parse_constants(f.read())["MAX_TICKET_GROUPS"] == L["MAX_GROUPS"]
    # the grid cases: 64 / 65 and 128 / 129 workgroups lie below MAX_GRID, the tiles of the four element types divide the row counts
    assert 2 * L["GROUP_SIZE"] + 1 < L["MAX_GRID"]
    # single-pass window: one constant for the real and the complex types (the cases use m = PIPE_CH, PIPE_CH + 1 for all four), below
    # the two-kernel window, which is below the batched driver's m <= 2 LOWSYNC_MAX and the pipelined recurrence's PL_MAX_M
    assert L["PIPE_CH"] == L["PIPE_CH_CPLX"] and L["PIPE_CH"] % 16 == 0            # (the resident kernel: P = PIPE_CH / 16 parts)
    assert L["PIPE_CH"] + 1 < 40 < L["LOWSYNC_MAX"] < 70 < 2 * L["LOWSYNC_MAX"]    # iop = 31 / 32 at m = 40, iop = 64 / 65 at m = 70
    assert L["PL_MAX_M"] == 2 * L["LOWSYNC_MAX"]
    # pattern analysis: the halo form's diagonals fit its reach; the general form holds more; the SELL halo needs a reach of its own
    assert L["PIPE_DIA_MAX"] <= 2 * L["PIPE_WMAX"] and L["PIPE_DIA_MAX"] + 1 <= 2 * L["PIPE_WMAX"] + 1 < L["GDIA_MAX"]
    assert 2 * L["PIPE_WMAX"] * 3 == 48                                            # pipelined Lanczos: n = 47 / 48
    # augmented operator: the single-pass and the two-kernel step take the same p (the kiops cases: p = 8 on either, p = 9 on neither)
    assert L["PIPE_AUG_MAX"] == L["FUSED_AUG_MAX"] and L["PIPE_AUG_MAX"] + 2 <= 10
    # combine kernels: a matrix of COEF_MAT_COLS columns by value holds the 32 rows of a full single-pass window; one column by value
    # holds the two-kernel window; the time stepper's six terms are the columns of the matrix form
    assert L["COEF_MAT_MAX"] // L["COEF_MAT_COLS"] >= 32 and L["COEF_MAT_MAX"] % L["COEF_MAT_COLS"] == 0
    assert L["COEF_BY_VALUE_MAX"] == L["LOWSYNC_MAX"] and L["COEF_MAT_COLS"] == 6
    # the step number travels in 11 bits; the continuation's one-launch reset holds CONT_SCALES_MAX scales, fewer than a long run has
    assert L["PIPE_MAX_STEPS"] < 2048 and L["PIPE_MAX_STEPS"] - 1 > 2 * L["LOWSYNC_MAX"]
    assert L["LOWSYNC_MAX"] < L["CONT_SCALES_MAX"] + 1 < 170
    # wave residency: 400 tiles of every real type stay below the grid limit's rows (the two limits are tested apart)
    assert limits.WAVE_TILES_MAX < L["MAX_GRID"]
    assert limits.tile_rows(8) == 512 and limits.tile_rows(4) == 1024 and limits.tile_rows(16) == 256
