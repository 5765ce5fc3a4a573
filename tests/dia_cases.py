"""Stored-diagonal (DIA / banded) test inputs and the position contract of expv_mi_op_create_dia_loc restated in numpy.

`expand` is the contract of include/expv_mi.h, nothing else: offsets with |k| >= n contribute nothing; the others, ascending,
give row i the entries with 0 <= i + k < n at column i + k; element (i, i + k) of the diagonal stored in row d of `data` is read
from slot i + k ("col"), i ("row") or min(i, i + k) ("start") of that row.  tests/test_dia_operator_cpu.py holds it against
scipy."""
import numpy as np
import scipy.sparse as sp

ALIGNS = ("col", "row", "start")
ALIGN_CODE = {"col": 0, "row": 1, "start": 2}
DTYPE_CODE = {"float64": 0, "complex128": 1, "float32": 2, "complex64": 3}


def slot(i, k, align):
    """where element (i, i + k) lies in its row of data"""
    return i + k if align == "col" else i if align == "row" else min(i, i + k)


def expand(data, offsets, n, align="col", ld=None):
    """(rowptr[n + 1], colind[nnz], vals[nnz], src[nnz]): the scalar CSR arrays, int64 / the dtype of data, and the element index
    into data (rows of ld elements) each position reads.  data may be None (vals is then None) when ld is given."""
    if ld is None:
        ld = np.asarray(data).shape[1]
    inr = sorted((int(k), d) for d, k in enumerate(offsets) if abs(int(k)) < n)
    rowptr, colind, src = [0], [], []
    for i in range(n):
        for k, d in inr:
            if 0 <= i + k < n:
                colind.append(i + k)
                src.append(d * ld + slot(i, k, align))
        rowptr.append(len(colind))
    src = np.asarray(src, dtype=np.int64)
    vals = None if data is None else np.asarray(data).reshape(-1)[src]
    return np.asarray(rowptr, dtype=np.int64), np.asarray(colind, dtype=np.int64), vals, src


def rowptr_closed_form(offsets, n):
    """the header's formula: rowptr[i] = sum_r clamp(min(i, n - s_r) - max(0, -s_r), 0, n - |s_r|)"""
    i = np.arange(n + 1, dtype=np.int64)
    out = np.zeros(n + 1, dtype=np.int64)
    for k in (int(k) for k in offsets if abs(int(k)) < n):
        out += np.clip(np.minimum(i, n - k) - max(0, -k), 0, n - abs(k))
    return out


def nnz_of(offsets, n):
    return sum(max(0, n - abs(int(k))) for k in offsets)


def min_ld(offsets, n, align):
    """the smallest ld the creator accepts"""
    need = 0
    for k in (int(k) for k in offsets if abs(int(k)) < n):
        need = max(need, (n if k > 0 else n + k) if align == "col" else (n - k if k >= 0 else n) if align == "row" else n - abs(k))
    return need


def scalar_matrix(data, offsets, n, align="col"):
    """the scipy csr_matrix of `expand`'s arrays, stored zeros kept"""
    rp, ci, va, _ = expand(data, offsets, n, align)
    return sp.csr_matrix((va, ci.astype(np.int32), rp.astype(np.int32)), shape=(n, n))


def random_values(shape, T, rng):
    v = rng.standard_normal(shape)
    if np.dtype(T).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v.astype(T)


def random_diagonals(offsets, n, T, seed=7):
    """{k: the n - |k| values of diagonal k, by ascending row}; out-of-range offsets get an empty vector"""
    rng = np.random.default_rng(seed)
    return {int(k): random_values(max(0, n - abs(int(k))), T, rng) for k in sorted(int(k) for k in offsets)}


def pack(diags, offsets, n, align, T, ld=None, fill=np.nan):
    """data[len(offsets)][ld] holding the diagonals of `diags` in the order of `offsets` under `align`; EVERY slot that corresponds
    to no matrix position -- the first / last |k| slots, everything up to ld, the whole row of an out-of-range offset -- holds
    `fill` (NaN: an operator that read one would not be finite)"""
    ld = max(min_ld(offsets, n, align), 1) if ld is None else ld
    data = np.full((len(offsets), ld), fill, dtype=T)
    for d, k in enumerate(int(k) for k in offsets):
        if abs(k) >= n:
            continue
        i = np.arange(max(0, -k), min(n, n - k))
        data[d, [slot(int(x), k, align) for x in i]] = diags[k]
    return data


def nan_padding(data, offsets, n, align):
    """a copy of data with every slot the contract does not read set to NaN"""
    data = np.asarray(data)
    _, _, _, src = expand(data, offsets, n, align)
    out = np.full(data.size, np.nan, dtype=data.dtype)
    out[src] = data.reshape(-1)[src]
    return out.reshape(data.shape)


def dense_of(diags, n, T):
    M = np.zeros((n, n), dtype=T)
    for k, v in diags.items():
        if abs(k) < n:
            i = np.arange(max(0, -k), min(n, n - k))
            M[i, i + k] = v
    return M


def scramble(offsets, seed=1):
    offsets = list(offsets)
    order = np.random.default_rng(seed).permutation(len(offsets))
    if len(offsets) > 1 and np.array_equal(order, np.arange(len(offsets))):
        order = order[::-1]
    return [offsets[j] for j in order]
