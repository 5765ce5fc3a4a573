"""Digest of the four truncated-Taylor entries (expv_taylor, expv_taylor_block, expv_taylor_grid, phiv_taylor): one line per call
with a hash of the result and a hash of its info dictionary, for the bit-for-bit comparison of two builds:

    python tools/taylor_digest.py > new.txt;  EXPV_MI_LIB=<other libexpv_mi.so> python tools/taylor_digest.py > old.txt;  diff old.txt new.txt

Inputs come from the seeded host generators of the tests (tests/expv_taylor_cases.py, tests/phiv_taylor_cases.py,
tests/expv_taylor_grid_cases.py, tests/taylor_dia_cases.py); nothing is drawn on the device.  Coverage: every element type; both
precisions; a band in the general diagonal form and the same band read from SELL slots (dia = 0), a random sparse operator (SELL),
one with rows that overflow SELL and a dense one (both: mul! + update pass), a reordered band, a many-diagonal operator;
n = 1, 65, 129, 257 (64 N + 1 for every pack width), 513, 20000; alpha = 40 (s > 1, early stops), alpha = 0, b = 0, a complex t on
a complex operator with a complex trace."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import expv_mi_loader
from tests import expv_taylor_cases as tc
from tests import expv_taylor_grid_cases as gc
from tests import phiv_taylor_cases as pc
from tests import taylor_dia_cases as dc

eu = expv_mi_loader.load()
SIZES = (1, 65, 129, 257, 513, 20000)
DENSE_MAX = 513
BLOCK_COLS = (1, 3, 8, 9)
PHIV = ((0, False), (1, False), (3, False), (3, True))      # (p, only u_p non-zero)


def h(x):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(x)).tobytes()).hexdigest()[:16]


def hd(info):
    return hashlib.sha256(repr(sorted(info.items())).encode()).hexdigest()[:16]


def context(**options):
    ctx = eu.Context()
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


CTX = {"dia0": context(dia=0), "reorder": context(reorder=2)}


def operators(n, T):
    """(name, operator as the entries take it, the matrix for t_for)"""
    A = tc.penta(n, T)
    yield "band", eu.MIOperator(A), A
    yield "band dia0", eu.MIOperator(A, CTX["dia0"]), A
    A = tc.random8(n, T)
    yield "random8", eu.MIOperator(A), A
    if n >= 65:
        A = tc.powerlaw(n, T)
        yield "powerlaw", eu.MIOperator(A), A
    if n <= DENSE_MAX:
        A = tc.dense(n, T)
        yield "dense", A, A
    if n >= 513:
        A, _ = tc.shuffled_band(n, T)
        A.sort_indices()
        yield "reordered", eu.MIOperator(A, CTX["reorder"]), A
    if n == 257:
        A = dc.BY_NAME["nd=9"].operator(T)
        yield "nd=9", eu.MIOperator(A), A


def grid_times(s):
    """0, nine interior outputs of stage 0 (two panels), the end of stage 0, an interior output of a later stage, R"""
    r = [0.0] + [j / (10.0 * s) for j in range(1, 10)] + [1.0 / s]
    if s > 1:
        r.append(1.5 / s)
    return np.array(r + [1.0])


def entries(tag, op, n, T, t, prec, b=None):
    b = tc.vector(n, T) if b is None else b
    kw = dict(precision=prec, return_info=True)
    w, info = eu.expv_taylor(t, op, b, **kw)
    print("%s expv_taylor %s %s" % (tag, h(w), hd(info)))
    for p in BLOCK_COLS:
        B = np.asfortranarray(np.stack([b if k == 0 else tc.vector(n, T, seed=k) for k in range(p)], axis=1))
        W, bi = eu.expv_taylor_block(t, op, B, **kw)
        print("%s expv_taylor_block p=%d %s %s" % (tag, p, h(W), hd(bi)))
    W, gi = eu.expv_taylor_grid(grid_times(info["s"]), op, b, t=t, **kw)
    print("%s expv_taylor_grid nt=%d qmax=%d accum=%d %s %s" % (tag, W.shape[1], gi["qmax"], gi["accumulate_launches"], h(W), hd(gi)))
    for p, only_last in PHIV:
        B = pc.block(n, p, T, only_last=only_last)
        if p == 0:
            B[:, 0] = b
        w, pi = eu.phiv_taylor(t, op, B, **kw)
        print("%s phiv_taylor p=%d%s %s %s" % (tag, p, " only u_p" if only_last else "", h(w), hd(pi)))


def main():
    for T in tc.DTYPES:
        name = np.dtype(T).name
        for n in SIZES:
            for oname, op, A in operators(n, T):
                t = tc.t_for(A, 40.0)
                for prec in ((0, 1) if n == 513 else (0,)):
                    entries("%-10s n=%-5d %-10s prec=%d" % (name, n, oname, prec), op, n, T, t, prec)
                if n != 257 or oname not in ("band", "random8", "dense"):
                    continue
                tag = "%-10s n=%-5d %-10s" % (name, n, oname)
                entries(tag + " alpha=0", op, n, T, 0.0, 0)
                entries(tag + " b=0    ", op, n, T, t, 0, b=np.zeros(n, dtype=T))
                if np.dtype(T).kind == "c":
                    entries(tag + " cplx t ", op, n, T, tc.t_for(A, 40.0, complex_t=True), 0)


if __name__ == "__main__":
    main()
