"""The constant-tile rule of the banded Float64 form, on the host: the numpy restatement (tests/elide_cases.py) against counts worked out
by hand, and the places the library declares the feature.  The device side is tests/test_gpu_elide_const_tiles.py."""
import os
import re

import numpy as np
import pytest

from tests import elide_cases as ec
from tests._util import C2_OFFSETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask(name, **kw):
    return ec.tile_mask(ec.stored_diagonals(ec.case(name, **kw), C2_OFFSETS))


def _pairs(mask):
    return int(sum(bin(int(b)).count("1") for b in mask))


@pytest.mark.parametrize("name", sorted(ec.EXPECTED_PAIRS))
def test_restated_mask_gives_the_counts_worked_out_by_hand(name):
    mask = _mask(name)
    assert mask.shape == (4,) and _pairs(mask) == ec.EXPECTED_PAIRS[name], (name, [bin(b) for b in mask])
    assert mask[3] == (0b10000 if name == "d" else 0)      # the ragged tile: zero fill (only a +0.0 diagonal is constant there)
    assert mask[0] & 0b00011 == 0                           # first tile of the sub-diagonals: rows without an entry


def test_zero_fill_decides_the_edge_tiles():
    a = _mask("a")
    assert list(a) == [0b11100, 0b11111, 0b11111, 0]
    even = _mask("a", n=ec.N_EVEN)                          # whole tiles: the super-diagonals end inside the last one
    assert list(even) == [0b11100, 0b11111, 0b11111, 0b00111]


def test_single_changes_clear_single_bits():
    a = _mask("a")
    assert list(_mask("b") ^ a) == [0, 0b00100, 0, 0]       # one interior entry of the main diagonal
    assert list(_mask("c")) == list(a)                      # a value change AT a tile boundary: both tiles constant
    assert list(_mask("c", sym=True) ^ a) == [0, 0, 0b00010, 0]      # (the sub-diagonal's change lands one row inside tile 2)
    assert list(_mask("d") ^ a) == [0, 0b10000, 0, 0b10000]  # -0.0 among +0.0 clears; the +0.0 diagonal matches its own zero fill
    assert list(_mask("nan") ^ a) == [0, 0b00100, 0, 0]
    assert not _mask("e").any()


def test_signed_zero_and_nan_payloads_are_compared_as_bits():
    s = np.full((1, ec.TILE), 0.0)
    assert ec.tile_mask(s)[0] == 1
    s[0, 17] = -0.0
    assert ec.tile_mask(s)[0] == 0
    s[:] = np.nan                                           # simplest rule: any NaN -> not constant, equal payloads or not
    assert ec.tile_mask(s)[0] == 0


def test_tenth_perturbed_operator_keeps_nine_tenths():
    n = 40 * ec.TILE + 5
    m = ec.tile_mask(ec.stored_diagonals(ec.tenth_perturbed(n), C2_OFFSETS))
    full = ec.tile_mask(ec.stored_diagonals(ec.case("a", n=n), C2_OFFSETS))
    assert _pairs(full) - _pairs(m) == 4 and all((f ^ p) in (0, 0b00100) for f, p in zip(full, m))


def test_the_feature_is_declared_where_callers_look():
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    assert re.search(r"int expv_mi_op_elide_info\(expv_mi_op_t op, int64_t out\[4\], unsigned char \*mask, int64_t mask_len\);", hdr)
    assert '"elide" 1' in hdr
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "_lib.py")).read()
    assert '"expv_mi_op_elide_info"' in src
    eng = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "engine_core.hip")).read()
    assert 'n == "elide"' in eng and "EXPV_MI_ELIDE" in eng
