#!/usr/bin/env python
"""Time gat-compare's single-file mode on a synthetic counts matrix (default 1 000 annotations x 10 000 samples: 499 500
pairs): pairs per second of the device path -- gat_compare_stats alone (k_compare_rows + k_null_stats over all pairs, the
matrix already uploaded) and gat_amd.compare.compare() end to end (upload, the call, one AnnotatorResult per pair) -- and
of the numpy path (gat_amd.compare.numpy_result, the reference's operations) on a random subsample of the pairs,
extrapolated to all of them.  Also the largest deviation of the device's mean / stddev / interval values from numpy's on
that subsample, in units of the bound the tests derive (tests/test_compare_gpu.py).

    python tools/time_compare.py [--annotations 1000] [--samples 10000] [--numpy-pairs 300] [--reps 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gat_amd                                   # noqa: E402
from gat_amd import compare as C                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--annotations", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--numpy-pairs", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_compare.txt"))
    a = ap.parse_args()
    rs = np.random.RandomState(2026)
    n, S = a.annotations, a.samples
    # counts of a run: per annotation a level and Poisson scatter around it; the observed value near the level
    level = rs.randint(200, 20000, n)
    m = rs.poisson(level[:, None], (n, S)).astype(np.float64)
    observed = np.maximum(1, (level * rs.uniform(0.6, 1.6, n)).astype(np.int64))
    rows = [gat_amd.AnnotatorResult("merged", "a%04d" % i, "na", float(o), r) for i, (o, r) in enumerate(zip(observed, m))]
    pairs = C.pairs_of([rows])
    ia, ib = np.triu_indices(n, 1)
    assert len(pairs) == len(ia) and pairs[n].data1 is rows[ia[n]] and pairs[n].data2 is rows[ib[n]]
    fold = np.array([x.fold for x in rows])
    ctx = gat_amd.get_context()
    ptr = ctx.alloc(m.nbytes)
    ctx.h2d(ptr, m)
    t_dev = []
    for _ in range(a.reps + 1):                                        # (the first call warms up: not counted)
        t0 = time.perf_counter()
        st = ctx.compare_stats(ptr, n, ptr, n, S, ia, ib, observed[ia], observed[ib], fold[ib] - fold[ia], 1.0)
        t_dev.append(time.perf_counter() - t0)
    ctx.free(ptr)
    t_dev = sorted(t_dev[1:])
    os.environ["GAT_DEVICE_STATS"] = "1"
    t0 = time.perf_counter()
    results = C.compare([rows], ctx=ctx)
    t_all = time.perf_counter() - t0
    assert len(results) == len(pairs) and int(st[:, 6].sum()) == 0
    pick = rs.choice(len(pairs), min(a.numpy_pairs, len(pairs)), replace=False)
    t0 = time.perf_counter()
    model = [C.numpy_result(pairs[k], 1.0) for k in pick]
    t_np = (time.perf_counter() - t0) / len(pick)
    worst, flips = 0.0, 0
    for k, w in zip(pick, model):
        p = pairs[k]
        r = (p.data1.observed / (p.data1.samples + 1.0) + 0.0001) / (p.data2.observed / (p.data2.samples + 1.0) + 0.0001)
        e = 4 * np.spacing(np.maximum(np.abs(np.log(r)), abs(w.observed)))
        g = results[k]
        worst = max(worst, abs(g.expected - w.expected) / e.mean(), abs(g.stddev - w.stddev) / e.mean(),
                    abs(g.lower95 - w.lower95) / e.max(), abs(g.upper95 - w.upper95) / e.max())
        flips += g.pvalue != w.pvalue
    med = t_dev[len(t_dev) // 2]
    lines = [
        "gat-compare, single-file mode: %d annotations x %d samples = %d pairs, MI355X, one GPU" % (n, S, len(pairs)),
        "    python tools/time_compare.py --annotations %d --samples %d --numpy-pairs %d --reps %d" % (n, S, len(pick), a.reps),
        "gat_compare_stats (k_compare_rows + k_null_stats, matrix on the device; median of %d calls, lowest .. highest):" % a.reps,
        "    %.3f s  (%.3f .. %.3f)   %s pairs/s" % (med, t_dev[0], t_dev[-1], format(int(len(pairs) / med), ",d").replace(",", " ")),
        "compare() end to end (upload, the call, one AnnotatorResult per pair on the host):",
        "    %.3f s   %s pairs/s" % (t_all, format(int(len(pairs) / t_all), ",d").replace(",", " ")),
        "numpy path (the reference's operations), %d random pairs, extrapolated to all:" % len(pick),
        "    %.3f ms per pair   %s pairs/s   %.1f s for all pairs" % (t_np * 1e3, format(int(1 / t_np), ",d").replace(",", " "),
                                                                     t_np * len(pairs)),
        "device against numpy on those pairs: largest deviation of expected / stddev / CI95low / CI95high = %.3f of the derived"
        " bound (4 ulp per element); p-values that differ: %d" % (worst, flips),
    ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
