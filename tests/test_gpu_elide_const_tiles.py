"""Constant tiles of the banded Float64 form (context option "elide", default 1): a stored diagonal that holds one bit pattern on a
whole tile of 512 stored rows is read there as one entry by the halo form of the single-pass step instead of being streamed.

  * the mask and the counter the library computes (creation, every values update, every creator) against the numpy restatement of
    the rule (tests/elide_cases.py);
  * elide = 1 against elide = 0, bit for bit, on H, V and w: overlapped and serial forms, Arnoldi windows that end one step inside
    each larger window variant (m = 9, 17, 26), Lanczos, iop = 2, a continuation; w against the C oracle at 1e-12;
  * the same at n ~ 1e6, the smallest size class at which a workgroup owns more than one tile (the mask byte of a later tile is
    requested one tile ahead: a path no small n takes) -- bit equality only, one operator with a tenth of its tiles perturbed;
  * option interplay with "stencil": path words as tests/test_gpu_option_forms.py pins them, all four combinations bit-equal.

Note on the edge tiles: with diagonal d stored by ROW, the zero fill of a sub-diagonal sits at the top of its first tile and that of
a super-diagonal at the end of its last rows; at n = 3 * 512 + 37 the last tile of every diagonal is ragged (rows >= n are zero fill)
and the first tile of the SUPER-diagonals is whole and constant.  tests/test_elide_mask_rule.py has the n = 4 * 512 counterpart."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import elide_cases as ec
from tests._util import C2_OFFSETS, close
from tests.option_forms import context_with
from tests.test_gpu_device_operator import to_torch_sparse

pytestmark = pytest.mark.gpu
N, TOL = ec.N_SMALL, 1e-12
PIPE = frozenset({"pipeline", "overlapped"})
PIPE_SERIAL = frozenset({"pipeline"})


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _expected(A):
    mask = ec.tile_mask(ec.stored_diagonals(A, C2_OFFSETS))
    return mask, int(sum(bin(int(b)).count("1") for b in mask))


def _assert_mask(op, A, what):
    mask, pairs = _expected(A)
    info = op.elide_info
    print("[elide] %-40s mask %s pairs %d" % (what, [bin(int(b)) for b in info["mask"]], info["constant_pairs"]))
    assert info["tiles"] == len(mask) and info["diagonals"] == len(C2_OFFSETS), (what, info)
    assert np.array_equal(info["mask"], mask), (what, list(info["mask"]), list(mask))
    assert info["constant_pairs"] == pairs, (what, info["constant_pairs"], pairs)
    return info


# ------------------------------------------------------------------ the mask ---------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "nan"])
def test_mask_matches_the_numpy_restatement(eu, name):
    A = ec.case(name)
    info = _assert_mask(eu.MIOperator(A, eu.Context()), A, "case (%s)" % name)
    assert info["constant_pairs"] == ec.EXPECTED_PAIRS[name]
    assert info["wholly_constant"] == (name == "a")
    m = info["mask"]
    assert m[0] & 0b00011 == 0, "first tile of the sub-diagonals: zero fill"
    assert m[3] == (0b10000 if name == "d" else 0), "ragged last tile: zero fill"


def test_every_creator_gives_the_same_mask(eu, torch):
    A = ec.case("b")
    ctx = eu.Context()
    _assert_mask(eu.MIOperator(to_torch_sparse(torch, A), ctx), A, "device CSR")
    C = A.tocoo()
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()
    _assert_mask(eu.MIOperator.from_coo(dev(C.row.astype(np.int32)), dev(C.col.astype(np.int32)), dev(C.data), N, ctx=ctx), A, "device COO")
    data = np.zeros((len(C2_OFFSETS), N))
    for d, o in enumerate(C2_OFFSETS):          # scipy's alignment: element (i, i + o) at column i + o
        data[d, max(0, o):N + min(0, o)] = A.diagonal(o)
    _assert_mask(eu.MIOperator.from_dia(dev(data), np.array(C2_OFFSETS), N, align="col", ctx=ctx), A, "device DIA")


def test_operators_without_the_form_report_nothing(eu):
    A = ec.case("a").astype(np.complex128)
    info = eu.MIOperator(A, eu.Context()).elide_info
    assert info["constant_pairs"] == 0 and info["tiles"] == 0 and info["mask"].size == 0, info


# ------------------------------------------------------------------ bitwise neutrality -----------------------------------------
def _products(eu, ctx, A, S, b, n):
    """H, V, w of every call the option must not change, and the path words of the expv"""
    op, out = eu.MIOperator(A, ctx), {}
    for m in (9, 17, 26):
        K = eu.arnoldi(op, b, m=m, ishermitian=False)
        assert K.m == m and not K.wasbreakdown
        out["arnoldi m=%d H" % m], out["arnoldi m=%d V" % m] = np.array(K.getH()), np.array(K.getV())
        out["arnoldi m=%d w" % m] = np.array(eu.expv_(np.empty(n), 0.6, K))
    K = eu.arnoldi(op, b, m=17, iop=2, ishermitian=False)
    out["iop=2 H"], out["iop=2 V"] = np.array(K.getH()), np.array(K.getV())
    Kc = eu.KrylovSubspace(np.float64, np.float64, n, 9, 0, ctx)      # resize (starts a plain subspace afresh), 9 steps, then init = 9 up to 17
    eu.arnoldi_(Kc, op, b, m=9, ishermitian=False)
    Kc.resize(17)
    eu.arnoldi_(Kc, op, b, m=9, ishermitian=False)
    eu.arnoldi_(Kc, op, b, m=17, ishermitian=False, init=9)
    out["continuation H"], out["continuation V"] = np.array(Kc.getH()), np.array(Kc.getV())
    out["continuation w"] = np.array(eu.expv_(np.empty(n), 0.6, Kc))
    if S is not None:
        opS = eu.MIOperator(S, ctx)
        K = eu.arnoldi(opS, b, m=17, ishermitian=True)
        out["lanczos H"], out["lanczos V"] = np.array(K.getH()), np.array(K.getV())
        out["lanczos w"] = np.array(eu.expv_(np.empty(n), 0.6, K))
    w = np.array(eu.expv(0.6, op, b, m=26, ishermitian=False))
    out["expv w"] = w
    c = ctx.counters()
    assert c["redo_serial"] == 0 and c["redo_wave_off"] == 0, c
    return out, frozenset(eu.expv.last_stats["path"]), op


def _assert_same(ra, rb, what):
    bad = [k for k in ra if not np.array_equal(ra[k], rb[k])]
    assert not bad, "%s: not bit-identical: %s" % (what, {k: float(np.max(np.abs(ra[k] - rb[k]))) for k in bad})


_ORACLE = {}


def _oracle_w(name, A, S, b):
    """w of the C restatement, once per case: Arnoldi m = 9, 17, 26 and Lanczos m = 17"""
    if name not in _ORACLE:
        o = {"arnoldi m=%d w" % m: co.expv_csr(0.6, A, b, m=m)[0] for m in (9, 17, 26)}
        o["lanczos w"] = co.expv_csr(0.6, S, b, m=17, hermitian=True)[0]
        _ORACLE[name] = o
    return _ORACLE[name]


@pytest.mark.parametrize("serial", [0, 1], ids=["overlapped", "serial"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_elide_is_bitwise_neutral(eu, name, serial):
    A, S = ec.case(name), ec.case(name, sym=True)
    b = np.random.default_rng(3).standard_normal(N)
    opts = {"pipeline_serial": 1} if serial else {}
    on, path_on, op_on = _products(eu, context_with(eu, dict(opts, elide=1)), A, S, b, N)
    off, path_off, _ = _products(eu, context_with(eu, dict(opts, elide=0)), A, S, b, N)
    assert path_on == path_off == (PIPE_SERIAL if serial else PIPE), (path_on, path_off)
    assert op_on.elide_info["constant_pairs"] == ec.EXPECTED_PAIRS[name]      # (there was something to elide)
    _assert_same(on, off, "case (%s), %s" % (name, "serial" if serial else "overlapped"))
    for k, wo in _oracle_w(name, A, S, b).items():
        close(on[k], wo, TOL, "case (%s) %s vs C oracle" % (name, k))


@pytest.mark.parametrize("serial", [0, 1], ids=["overlapped", "serial"])
def test_elide_is_bitwise_neutral_where_a_workgroup_owns_several_tiles(eu, serial):
    """n ~ 1e6: 1954 tiles on at most 1024 resident workgroups -- 2 to 4 tiles per workgroup in the four window variants, which an
    Arnoldi run of 26 steps passes through one after the other.  A tenth of the tiles is perturbed, so set and clear bits alternate
    within a workgroup's tiles."""
    n = 1_000_000 + 37
    A = ec.tenth_perturbed(n)
    b = np.random.default_rng(4).standard_normal(n)
    opts = {"pipeline_serial": 1} if serial else {}
    res = []
    for elide in (1, 0):
        ctx = context_with(eu, dict(opts, elide=elide))
        op = eu.MIOperator(A, ctx)
        K = eu.arnoldi(op, b, m=26, ishermitian=False)
        r = {"H": np.array(K.getH()), "w": np.array(eu.expv_(np.empty(n), 0.6, K)), "V": np.array(K.getV())}
        K2 = eu.arnoldi(op, b, m=12, iop=2, ishermitian=False)
        r["iop=2 H"], r["iop=2 V last"] = np.array(K2.getH()), np.array(K2.getV())[:, -2:]
        res.append(r)
        if elide:
            info = op.elide_info
            tiles = (n + ec.TILE - 1) // ec.TILE
            print("[elide] n=%d: %d of %d (tile, diagonal) pairs constant" % (n, info["constant_pairs"], 5 * tiles))
            assert 0.85 * 5 * tiles < info["constant_pairs"] < 5 * tiles - 5
    _assert_same(res[0], res[1], "n = %d, %s" % (n, "serial" if serial else "overlapped"))


# ------------------------------------------------------------------ values updates ---------------------------------------------
def test_mask_and_results_follow_values_updates(eu):
    Aa, Ab = ec.case("a"), ec.case("b")
    b = np.random.default_rng(3).standard_normal(N)
    ctx = eu.Context()
    fresh = {}
    for name, A in (("a", Aa), ("b", Ab)):
        K = eu.arnoldi(eu.MIOperator(A, ctx), b, m=17, ishermitian=False)
        fresh[name] = {"H": np.array(K.getH()), "V": np.array(K.getV()), "w": np.array(eu.expv_(np.empty(N), 0.6, K))}
    op = eu.MIOperator(Aa.copy(), ctx)
    _assert_mask(op, Aa, "created as (a)")
    for name, A in (("b", Ab), ("a", Aa), ("b", Ab)):
        op.update_values(A)
        info = _assert_mask(op, A, "updated to (%s)" % name)
        assert info["constant_pairs"] == ec.EXPECTED_PAIRS[name] and info["wholly_constant"] == (name == "a")
        K = eu.arnoldi(op, b, m=17, ishermitian=False)
        got = {"H": np.array(K.getH()), "V": np.array(K.getV()), "w": np.array(eu.expv_(np.empty(N), 0.6, K))}
        _assert_same(got, fresh[name], "after the update to (%s) vs a freshly created operator" % name)


# ------------------------------------------------------------------ option interplay -------------------------------------------
def test_stencil_and_elide_options_combine(eu):
    A = ec.case("a")
    b = np.random.default_rng(3).standard_normal(N)
    res = {}
    for stencil in (0, 1):
        for elide in (0, 1):
            ctx = context_with(eu, {"stencil": stencil, "elide": elide})
            r, path, op = _products(eu, ctx, A, None, b, N)
            assert path == PIPE, (stencil, elide, sorted(path))      # (tests/test_gpu_option_forms.py: banded_const, default and stencil)
            assert op.elide_info["constant_pairs"] == 13 and op.elide_info["wholly_constant"]
            res[(stencil, elide)] = r
    for k in res:
        _assert_same(res[k], res[(0, 0)], "stencil = %d, elide = %d vs both off" % k)


def test_environment_switch_reaches_new_contexts(eu, monkeypatch):
    monkeypatch.setenv("EXPV_MI_ELIDE", "0")
    assert eu.Context().get_option("elide") == 0
    monkeypatch.delenv("EXPV_MI_ELIDE")
    assert eu.Context().get_option("elide") == 1
