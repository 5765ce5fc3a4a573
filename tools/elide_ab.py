"""Constant-tile elision (context option "elide") A/B: expv at n = 1e6, m = 30, Float64, on three five-diagonal operators --
  c2       the headline operator (every diagonal constant),
  random   random diagonals (no tile is constant: what the mask costs where it does not apply),
  tenth    c2 with one entry changed in every tenth tile (partial constancy).
One process times one tree with one setting; a driver interleaves processes of the trees to compare (parent checkout / this tree):

  python tools/elide_ab.py --tree . --elide 1 --label new
  python tools/elide_ab.py --tree ../parent --label parent          (a tree without the option: --elide is left out)

Each line: label, operator, constant (tile, diagonal) pairs where the tree reports them, the median / min / max ms per call over
--batches timings of --calls calls, and matvecs/s at the median."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--elide", type=int, default=None)
ap.add_argument("--label", default="tree")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--m", type=int, default=30)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--batches", type=int, default=5)
ap.add_argument("--ops", default="c2,random,tenth")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np
import scipy.sparse as sp
import torch
import expv_mi_loader

eu = expv_mi_loader.load()
n, m = args.n, args.m
OFFS, VALS = (-2, -1, 0, 1, 2), (0.3, 1.2, -2.0, 0.8, -0.1)


def operator(kind):
    rng = np.random.default_rng(11)
    D = [np.full(n - abs(o), v) for o, v in zip(OFFS, VALS)]
    if kind == "random":      # same scale as c2, every entry its own value
        D = [v * (1.0 + 0.1 * rng.standard_normal(len(d))) for d, v in zip(D, VALS)]
    elif kind == "tenth":
        for t in range(3, (n + 511) // 512 - 1, 10):
            D[2][t * 512 + 100] = -2.5
    return sp.diags(D, OFFS, shape=(n, n), format="csr")


b = torch.randn(n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
w = torch.empty_like(b)
for kind in args.ops.split(","):
    ctx = eu.Context(async_outputs=True)
    if args.elide is not None:
        ctx.set_option("elide", args.elide)
    op = eu.MIOperator(operator(kind), ctx)
    f = lambda: eu.expv(1.0, op, b, m=m, ishermitian=False, out=w)
    t_end = time.perf_counter() + 0.6      # clocks up
    while time.perf_counter() < t_end:
        f()
    ctx.sync()
    ts = []
    for _ in range(args.batches):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            f()
        ctx.sync()
        ts.append((time.perf_counter() - t0) / args.calls)
    ts.sort()
    med = ts[len(ts) // 2]
    pairs = op.elide_info["constant_pairs"] if hasattr(op, "elide_info") else None
    print(json.dumps({"label": args.label, "elide": args.elide, "operator": kind, "constant_pairs": pairs, "ms_median": round(1e3 * med, 4),
                      "ms_min": round(1e3 * ts[0], 4), "ms_max": round(1e3 * ts[-1], 4), "matvecs_per_s": round(m / med, 1),
                      "path": "+".join(sorted(eu.expv.last_stats["path"]))}), flush=True)
    del op, ctx
