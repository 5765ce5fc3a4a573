"""Linear combinations of operators built on the device (expv_mi_op_create_lincomb / expv_mi_op_lincomb_refresh;
MIOperator.lincomb, .recombine, + - * /): the reference's expv(t, H0 + f*H1, b) and expv(t, A - sigma*I, b).

The yardstick is the operator expv_mi_op_create_csr_loc makes, on the same context, of the CSR arrays of the combination as
tests/lincomb_cases.py: lincomb_arrays states them (held against scipy in tests/test_lincomb_cpu.py): from the checked arrays on the
two take the same tail, so nnz, ishermitian, opnorm_inf, ingest / reorder / patch info, matvec and arnoldi / expv / phiv are
compared for bit equality.  Dense terms are held against the dense operator of the host sum under the same roundings."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import adjoint_cases as ac
from tests import bsr_cases as bc
from tests import coo_cases as cc
from tests import dia_cases as dc
from tests import lincomb_cases as lc
from tests.test_gpu_adjoint_operator import csr_loc
from tests.test_gpu_bsr_operator import bsr_op, ingest, same_everything
from tests.test_gpu_device_operator import DTYPES, make_pattern, to_torch_sparse
from tests.test_gpu_dia_operator import on_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def term_op(eu, torch, ctx, term):
    """the operator of a term's arrays as they stand (unsorted rows and repeats included), made from device arrays"""
    rp, ci, va = term
    n = len(rp) - 1
    if len(ci) == 0:
        return eu.MIOperator(sp.csr_matrix((n, n), dtype=va.dtype), ctx)
    At = torch.sparse_csr_tensor(torch.as_tensor(np.asarray(rp)), torch.as_tensor(np.asarray(ci)), torch.as_tensor(np.asarray(va)), size=(n, n)).cuda()
    return eu.MIOperator(At, ctx)


def twin(eu, ctx, terms, coefs, identity=None):
    """the definition: the CSR-born operator of the restatement's arrays"""
    return csr_loc(eu, ctx, *lc.lincomb_arrays(terms, coefs, identity))


def same_operator(eu, ctx, op, ref, T, what, m=25):
    same_everything(eu, ctx, op, ref, T, what, m=m)
    assert (op.nnz, op.ishermitian, op.opnorm_inf) == (ref.nnz, ref.ishermitian, ref.opnorm_inf), what
    assert ingest(op) == ingest(ref), (what, ingest(op), ingest(ref))
    r1, r2 = dict(op.reorder_info), dict(ref.reorder_info)
    r1.pop("setup_s"), r2.pop("setup_s")
    assert r1 == r2, (what, r1, r2)


# ------------------------------------------------------------------ 1. every case, every element type: the CSR-born twin, bit for bit
# n = 1 and 37; 1500 and 1501: every term holds more than 4096 stored entries (the key kernel's tile and the sort's), and the
# result's nnz at 1501 is odd (two_bands: 9 n - 24), so the last pack of the gather-scale-sum is a partial one for every element type
SIZES = [1, 37, 1500, 1501]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_every_case_is_the_csr_born_twin_bit_for_bit(eu, torch, case, T, n):
    terms = lc.CASES[case](n, T)
    ctx = eu.Context()
    ops = [term_op(eu, torch, ctx, t) for t in terms]
    if case == "own_adjoint":
        ops[1] = ops[0].adjoint()                # the term the library made itself
    if case == "repeated":
        assert ops[0].nnz == len(terms[0][1]), "the repeats are stored"
    if n >= 1500 and case != "zero_term":
        assert all(o.nnz > 4096 for o in ops)
    for coefs, identity in lc.coefficient_sets(len(terms), T):
        what = "%s %s n=%d %s + %s I" % (case, np.dtype(T).name, n, coefs, identity)
        op = eu.MIOperator.lincomb(ops, coefs, identity)
        rp, ci, va = lc.lincomb_arrays(terms, coefs, identity)
        assert op.src is None and op.shape == (n, n) and op.dtype == np.dtype(T) and op.nnz == len(ci), what
        if case == "two_bands" and n == 1501:
            assert op.nnz == 9 * n - 24 and op.nnz % 2 == 1
        same_operator(eu, ctx, op, csr_loc(eu, ctx, rp, ci, va), T, what)
        info = op.ingest_info
        assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (n + 1 + op.nnz) and info["value_bytes_to_host"] == 0, info
        assert info["coo_entries"] == 0 and info["sort_passes"] == 0, info


# ------------------------------------------------------------------ 2. a term stored reordered, a term in patch form
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_a_reordered_term_and_a_term_in_patch_form(eu, torch, T):
    ctx = eu.Context()
    A, B = make_pattern("c2_permuted", T), make_pattern("c2", T)
    pa, pb = eu.MIOperator(to_torch_sparse(torch, A), ctx), eu.MIOperator(to_torch_sparse(torch, B), ctx)
    assert pa.reorder_info["reordered"]
    coefs, identity = ([1.5, -2.0], 0.25) if np.dtype(T).kind != "c" else ([1.5 - 0.5j, -2.0], 0.25j)
    op = eu.MIOperator.lincomb([pa, pb], coefs, identity)
    same_operator(eu, ctx, op, twin(eu, ctx, [lc.arrays(A), lc.arrays(B)], coefs, identity), T, "reordered term %s" % np.dtype(T).name)
    G = make_pattern("grid", T)
    pg = eu.MIOperator(to_torch_sparse(torch, G), ctx)
    assert pg.patch_info["patch_form"]
    g = lc.arrays(G)
    gh = ac.adjoint_arrays(*g, True)[:3]
    op = eu.MIOperator.lincomb([pg, pg.adjoint(), pg], [1.0, -0.5, 0.25])
    same_operator(eu, ctx, op, twin(eu, ctx, [g, gh, g], [1.0, -0.5, 0.25]), T, "patch-form term %s" % np.dtype(T).name)


# ------------------------------------------------------------------ 3. every birth of a term
@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("birth", ["host_csr", "host_csc", "device_csr", "device_csc", "coo", "bsr", "dia", "adjoint"])
def test_every_birth_of_a_term(eu, torch, birth, T):
    ctx = eu.Context()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    if birth == "coo":          # shuffled triplets with repeats: summed at creation, duplicate-free once stored
        n = 200
        row, col, vals = cc.random_triplets(n, 900, T, seed=12, repeat_share=0.15, ends=True)
        parent = eu.MIOperator.from_coo(dev(row), dev(col), dev(vals), n, ctx=ctx)
        M = cc.expected_csr(row, col, vals, n)
    elif birth == "bsr":
        ptr, idx, vals = bc.block_tridiagonal(40, 3, T)
        parent = bsr_op(eu, torch, ctx, ptr, idx, vals)
        M = bc.scalar_matrix(ptr, idx, vals, 3)
    elif birth == "dia":
        n, offs = 300, dc.scramble([-17, -1, 0, 1, 17])
        data = dc.pack(dc.random_diagonals(offs, n, T), offs, n, "col", T)
        parent = eu.MIOperator.from_dia(on_device(torch, data), offs, n, "col", ctx=ctx)
        M = dc.scalar_matrix(data, offs, n, "col")
    elif birth == "adjoint":
        S = ac.upper(257, T)
        parent = eu.MIOperator(to_torch_sparse(torch, S), ctx).adjoint()
        M = S.conj().T
    elif birth.startswith("device"):
        M = ac.upper(257, T)
        parent = eu.MIOperator(to_torch_sparse(torch, M, fmt=birth[-3:]), ctx)
    else:
        M = ac.upper(257, T)
        parent = eu.MIOperator(M.tocsc() if birth == "host_csc" else M, ctx)
    M = sp.csr_matrix(M).astype(T)
    M.sort_indices()
    n = M.shape[0]
    assert parent.nnz == M.nnz
    B = ac.band(n, T, 31)
    other = eu.MIOperator(to_torch_sparse(torch, B), ctx)
    coefs = [-1.5, 2.0] if np.dtype(T).kind != "c" else [-1.5 + 1.0j, 2.0]
    for order in (0, 1):
        ops, terms = [parent, other][::1 - 2 * order], [lc.arrays(M), lc.arrays(B)][::1 - 2 * order]
        op = eu.MIOperator.lincomb(ops, coefs, identity=0.5)
        same_operator(eu, ctx, op, twin(eu, ctx, terms, coefs, 0.5), T, "%s %s order %d" % (birth, np.dtype(T).name, order))


# ------------------------------------------------------------------ 4. recombine
@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("identity", [None, -0.75])
def test_recombine_is_lincomb_anew(eu, torch, T, identity):
    n = 1501
    ta, tb = lc.two_bands(n, T)
    ctx = eu.Context()
    a, b = term_op(eu, torch, ctx, ta), term_op(eu, torch, ctx, tb)
    comb = eu.MIOperator.lincomb([a, b], [1.0, 1.0], identity)
    c2 = [0.5, -3.0] if np.dtype(T).kind != "c" else [0.5 + 2.0j, -3.0]
    i2 = None if identity is None else 2.5
    assert comb.recombine(c2, identity=i2) is comb
    what = "recombine %s identity %s" % (np.dtype(T).name, identity)
    same_operator(eu, ctx, comb, eu.MIOperator.lincomb([a, b], c2, i2), T, what + ": new coefficients")
    same_operator(eu, ctx, comb, twin(eu, ctx, [ta, tb], c2, i2), T, what + ": new coefficients vs twin", m=10)
    # the terms' values change through update_values; the kept terms are read again
    vb = ac.int_values(len(tb[1]), T, np.random.default_rng(77))
    b.update_values(torch.as_tensor(vb).cuda())
    comb.recombine(c2, identity=i2)
    tb2 = (tb[0], tb[1], vb)
    same_operator(eu, ctx, comb, eu.MIOperator.lincomb([a, b], c2, i2), T, what + ": new values")
    same_operator(eu, ctx, comb, twin(eu, ctx, [ta, tb2], c2, i2), T, what + ": new values vs twin", m=10)
    # other operators of the same patterns, and back to back: the same bits
    b3 = term_op(eu, torch, ctx, tb2)
    x = ac.int_vector(n, T, 3)
    y0 = np.array(comb.matvec(x))
    for _ in range(2):
        comb.recombine(c2, terms=[a, b3], identity=i2)
        assert np.array_equal(np.array(comb.matvec(x)), y0)
    assert np.array_equal(np.array(eu.expv(0.3, comb, x, m=20)), np.array(eu.expv(0.3, twin(eu, ctx, [ta, tb2], c2, i2), x, m=20)))
    # the identity's coefficient defaults to the last one given; without the identity there is none to give
    if identity is None:
        with pytest.raises(ValueError, match="without the identity"):
            comb.recombine(c2, identity=1.0)
    else:
        comb.recombine(c2)
        assert np.array_equal(np.array(comb.matvec(x)), y0)


def test_recombine_refusals(eu, torch):
    T = np.float64
    n = 300
    ta, tb = lc.two_bands(n, T)
    ctx = eu.Context()
    a, b = term_op(eu, torch, ctx, ta), term_op(eu, torch, ctx, tb)
    comb = a + b
    with pytest.raises(eu.ExpvMIError, match="op_lincomb_refresh.*number of terms"):
        comb.recombine([1.0, 1.0, 1.0], terms=[a, b, a])
    with pytest.raises(ValueError, match="one coefficient per term"):
        comb.recombine([1.0])
    with pytest.raises(eu.ExpvMIError, match="op_lincomb_refresh.*differs"):      # another element type
        comb.recombine([1.0, 1.0], terms=[a, term_op(eu, torch, ctx, lc.two_bands(n, np.float32)[1])])
    with pytest.raises(eu.ExpvMIError, match="op_lincomb_refresh.*differs"):      # another nnz in the second place
        comb.recombine([1.0, 1.0], terms=[a, term_op(eu, torch, ctx, lc.arrays(ac.upper(n, T)))])
    with pytest.raises(eu.ExpvMIError, match="op_lincomb_refresh.*another context"):
        comb.recombine([1.0, 1.0], terms=[a, term_op(eu, torch, eu.Context(), tb)])
    with pytest.raises(eu.ExpvMIError, match="op_lincomb_refresh.*not finite"):
        comb.recombine([1.0, float("inf")])
    with pytest.raises(TypeError, match="lincomb"):
        a.recombine([1.0])
    lib = eu._lib.load()
    h = (C.c_void_p * 1)(a._h)
    one = np.array([1.0, 0.0])
    assert lib.expv_mi_op_lincomb_refresh(a._h, 1, h, one.ctypes.data) == 2 and b"not created by op_create_lincomb" in lib.expv_mi_last_error(ctx._h)
    # astype and the matrix forms of update_values point to the terms
    with pytest.raises(TypeError, match="combine the converted terms"):
        comb.astype(np.complex128)
    with pytest.raises(TypeError, match="recombine"):
        comb.update_values(lc.matrix(ta))
    # bare values in the result's own sorted-row order are the ordinary value update
    rp, ci, va = lc.lincomb_arrays([ta, tb], [2.0, -1.0])
    comb.update_values(va)
    same_operator(eu, ctx, comb, csr_loc(eu, ctx, rp, ci, va), T, "update_values in the result's order")


# ------------------------------------------------------------------ 5. the driven Hamiltonian: H0 + f H1 over a few f, then expv
@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_driven_operator_through_recombine_then_expv(eu, torch, T):
    n = 1500
    t0, t1 = lc.two_bands(n, T)
    t0 = (t0[0], t0[1], (t0[2] / 8).astype(T))      # (a smaller norm: a short Krylov run)
    t1 = (t1[0], t1[1], (t1[2] / 8).astype(T))
    ctx = eu.Context()
    h0, h1 = term_op(eu, torch, ctx, t0), term_op(eu, torch, ctx, t1)
    b = np.random.default_rng(5).standard_normal(n).astype(T)
    H = eu.MIOperator.lincomb([h0, h1], [1.0, 0.0])
    for f in (0.0, 0.3, -1.25, 1e-3, 7.0):
        H.recombine([1.0, f])
        ref = twin(eu, ctx, [t0, t1], [1.0, f])
        assert H.opnorm_inf == ref.opnorm_inf and H.ishermitian == ref.ishermitian
        assert np.array_equal(np.array(eu.expv(0.1, H, b)), np.array(eu.expv(0.1, ref, b))), f


# ------------------------------------------------------------------ 6. dense terms
def padded_term(torch, n, T, pad, seed, shift):
    """(flat, view, host): an n x n column-major device view with leading dimension n + pad that starts `shift` elements into its
    buffer (shift = 1: not 16-byte aligned for the 4- and 8-byte element types); everything outside the matrix holds NaN"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if np.dtype(T).kind == "c" else 0)).astype(T)
    flat = torch.full((n * (n + pad) + shift,), float("nan"), dtype=torch.as_tensor(np.zeros(1, dtype=T)).dtype, device="cuda")
    view = flat[shift:].view(n, n + pad).t()[:n, :]      # element (i, j) at shift + j (n + pad) + i
    view.copy_(torch.as_tensor(a))
    return flat, view, a


def host_combination(mats, coefs, identity):
    """the dense combination under the contract's roundings"""
    acc = lc.scaled(coefs[0], mats[0])
    for c, m in zip(coefs[1:], mats[1:]):
        acc = acc + lc.scaled(c, m)
    if identity is not None:
        T = acc.dtype
        R = lc.real_type(T)
        c = complex(identity)
        d = np.arange(acc.shape[0])
        acc[d, d] = acc[d, d] + (T.type(R(c.real) + 1j * R(c.imag)) if T.kind == "c" else T.type(R(c.real)))
    return acc


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("n", [5, 130])
def test_dense_terms_give_the_dense_operator_of_the_host_sum(eu, torch, n, T):
    ctx = eu.Context()
    parts = [padded_term(torch, n, T, pad, seed, shift) for pad, seed, shift in ((3, 1, 1), (0, 2, 0), (2, 3, 1))]
    before = [p[0].cpu().numpy().tobytes() for p in parts]
    ops = [eu.MIOperator(p[1], ctx) for p in parts]
    mats = [p[2] for p in parts]
    x = np.random.default_rng(1).standard_normal(n).astype(T)
    for coefs, identity in lc.coefficient_sets(3, T):
        what = "dense n=%d %s %s + %s I" % (n, np.dtype(T).name, coefs, identity)
        op = eu.MIOperator.lincomb(ops, coefs, identity)
        want = host_combination(mats, coefs, identity)
        packed = torch.as_tensor(np.ascontiguousarray(want.T)).cuda().t()      # column-major, leading dimension n
        ref = eu.MIOperator(packed, ctx)
        assert np.isfinite(op.opnorm_inf), what + ": padding was read"
        same_everything(eu, ctx, op, ref, T, what)
        assert np.array_equal(np.array(eu.expv(0.2, op, x)), np.array(eu.expv(0.2, ref, x))), what
    assert [p[0].cpu().numpy().tobytes() for p in parts] == before, "the terms and their padding are unchanged"
    # the identity touches the diagonal only
    plain, shifted = eu.MIOperator.lincomb(ops[:1], [1.0]), eu.MIOperator.lincomb(ops[:1], [1.0], identity=3.0)
    for j in range(min(n, 7)):
        e = np.zeros(n, dtype=T)
        e[j] = 1
        col, col3 = np.array(plain.matvec(e)), np.array(shifted.matvec(e))
        assert np.array_equal(col, mats[0][:, j])
        assert np.array_equal(np.delete(col3, j), np.delete(col, j)) and col3[j] == mats[0][j, j] + T(3.0)
    # the result owns its matrix; recombine reads the terms again
    y0 = np.array(op.matvec(x))
    parts[0][1].zero_()
    torch.cuda.synchronize()
    assert np.array_equal(np.array(op.matvec(x)), y0)
    op.recombine(coefs, identity=identity)
    mats[0] = np.zeros_like(mats[0])
    want = host_combination(mats, coefs, identity)
    ref = eu.MIOperator(torch.as_tensor(np.ascontiguousarray(want.T)).cuda().t(), ctx)
    same_everything(eu, ctx, op, ref, T, "dense recombine n=%d %s" % (n, np.dtype(T).name))
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*do not mix"):
        eu.MIOperator.lincomb([ops[0], eu.MIOperator(ac.band(n, T), ctx)], [1.0, 1.0])


# ------------------------------------------------------------------ 7 - 8. refusals and the cap
def test_matrix_free_terms_and_the_cap(eu, torch):
    ctx = eu.Context()
    T = np.float64
    a = eu.MIOperator(ac.band(16, T), ctx)
    free = eu.MIOperator(None, ctx, matvec=lambda x: 2 * x, shape=(16, 16), dtype=T)
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb") as e:
        eu.MIOperator.lincomb([a, free], [1.0, 1.0])
    assert e.value.kind == "Unsupported"
    eight = eu.MIOperator.lincomb([a] * 8, [1.0] * 8)      # the same handle eight times
    same_operator(eu, ctx, eight, twin(eu, ctx, [lc.arrays(ac.band(16, T))] * 8, [1.0] * 8), T, "8 x the same handle")
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*nterms"):
        eu.MIOperator.lincomb([a] * 9, [1.0] * 9)
    # the identity without a term: this call has no context, element type or size to make c I of
    with pytest.raises(ValueError, match="one term at least"):
        eu.MIOperator.lincomb([], [], identity=2.0)
    lib = eu._lib.load()
    out, pair = C.c_void_p(0x1234), np.array([2.0, 0.0])
    assert lib.expv_mi_op_create_lincomb(0, None, pair.ctypes.data, 1, C.byref(out)) == 2 and out.value == 0x1234
    # the other refusals that need operators
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*differ in context, dtype or n"):
        eu.MIOperator.lincomb([a, eu.MIOperator(ac.band(17, T), ctx)], [1.0, 1.0])
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*differ in context, dtype or n"):
        eu.MIOperator.lincomb([a, eu.MIOperator(ac.band(16, np.float32), ctx)], [1.0, 1.0])
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*differ in context, dtype or n"):
        eu.MIOperator.lincomb([a, eu.MIOperator(ac.band(16, T), eu.Context())], [1.0, 1.0])
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*imaginary"):
        eu.MIOperator.lincomb([a], [1.0j])
    with pytest.raises(eu.ExpvMIError, match="op_create_lincomb.*not finite"):
        eu.MIOperator.lincomb([a], [1.0], identity=float("nan"))


# ------------------------------------------------------------------ 9. the plan cache is keyed by the combined pattern
def test_second_creation_of_a_pattern_takes_its_plan_from_the_cache(eu, torch):
    from tests._util import c2_operator
    from tests.test_gpu_parity import _shuffle
    A = _shuffle(c2_operator(30_000), 23)
    A.sort_indices()
    ctx = eu.Context()
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    eu.plan_cache(clear=True)
    first = eu.MIOperator.lincomb([parent, parent], [1.0, 0.5], identity=2.0)      # the parent's pattern: it stores its diagonal
    second = eu.MIOperator.lincomb([parent, parent], [-1.0, 0.25], identity=1.0)
    assert first.nnz == A.nnz and first.reorder_info["reordered"] and not first.ingest_info["plan_cached"]
    assert second.ingest_info["plan_cached"]
    second.recombine([1.0, 0.5], identity=2.0)
    same_everything(eu, ctx, second, first, np.float64, "plan from the cache")


# ------------------------------------------------------------------ 10 - 11. the Python operators
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_python_operators(eu, torch, T):
    n = 300
    ta, tb = lc.two_bands(n, T)
    ctx = eu.Context()
    a, b = term_op(eu, torch, ctx, ta), term_op(eu, torch, ctx, tb)
    x = ac.int_vector(n, T, 9)
    z = a - a
    assert z.nnz == a.nnz and z.opnorm_inf == 0.0 and not np.array(z.matvec(x)).any(), "A - A keeps the entries of A as stored zeros"
    two = 2 * a
    assert two.opnorm_inf == 2 * a.opnorm_inf and two.nnz == a.nnz
    same_operator(eu, ctx, two, a * 2.0, T, "2 A vs A 2")
    same_operator(eu, ctx, -a, eu.MIOperator.lincomb([a], [-1]), T, "-A vs lincomb([A], [-1])")
    same_operator(eu, ctx, -a, twin(eu, ctx, [ta], [-1.0]), T, "-A vs twin")
    same_operator(eu, ctx, a + b, twin(eu, ctx, [ta, tb], [1.0, 1.0]), T, "A + B")
    same_operator(eu, ctx, a - b, twin(eu, ctx, [ta, tb], [1.0, -1.0]), T, "A - B")
    same_operator(eu, ctx, a / 4, twin(eu, ctx, [ta], [0.25]), T, "A / 4")
    same_operator(eu, ctx, np.float32(0.5) * a, twin(eu, ctx, [ta], [0.5]), T, "numpy scalar * A")
    assert (a + b) is not (a + b) and (a + b).src is None
    for bad in (lambda: a + 1, lambda: 1 + a, lambda: a - 2.0, lambda: a * b, lambda: a * np.ones(n), lambda: np.ones(n) * a,
                lambda: a / b, lambda: 1 / a, lambda: a + lc.matrix(ta), lambda: a * "2", lambda: 3 - a, lambda: a * True):
        with pytest.raises(TypeError):
            bad()
