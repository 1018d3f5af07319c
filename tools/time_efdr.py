#!/usr/bin/env python
"""Time --qvalue-method=efdr (the resampling-based FDR, gat_amd/efdr.py) on synthetic count matrices: per shape the upload of
the float64 matrix, gat_efdr_counts on the resident matrix (host clock around the synchronous call) with the device time of
k_minp_rank and k_efdr separately (events, gat_efdr_times) -- with no level, with 8 levels, with the thresholds in chunks of
64, and on a matrix of rows of three distinct values (long ties: a whole wave on one LDS bin) --, the whole efdr.compute call
with two cutoffs (k_obs and stacking the rows on the host, upload, device, order and order statistics), and the numpy model of
tests/efdr_model.py on a subsample of the rows, scaled to all of them.  The counts of the subsample's family are checked
against the model.

    python tools/time_efdr.py [--rows 1000] [--samples 10000,100000] [--numpy-rows 40] [--reps 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gat_amd                                   # noqa: E402
import efdr_model as E                           # noqa: E402
from gat_amd import efdr, minp                   # noqa: E402


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def _timed(ctx, reps, ptr, R, S, ones, means, k_obs, levels):
    t_call, t_rank, t_efdr = [], [], []
    for _ in range(reps + 1):                                            # (the first call warms up: not counted)
        t0 = time.perf_counter()
        v, per = ctx.efdr_counts(ptr, R, S, ones, means, k_obs, levels)
        t_call.append(time.perf_counter() - t0)
        a, b = ctx.efdr_times()
        t_rank.append(a * 1e-3)
        t_efdr.append(b * 1e-3)
    return _median(t_call[1:]), _median(t_rank[1:]), _median(t_efdr[1:]), v


def shape(ctx, R, S, n_numpy, reps, rs):
    # counts of a run: per annotation a level and Poisson scatter around it; the observed value near the level
    level = rs.randint(200, 20000, R)
    m = rs.poisson(level[:, None], (R, S)).astype(np.float64)
    observed = np.maximum(1, (level * rs.uniform(0.97, 1.03, R)).astype(np.int64)).astype(np.float64)
    rows = [gat_amd.AnnotatorResult("merged", "a%04d" % i, "na", o, r) for i, (o, r) in enumerate(zip(observed, m))]
    means = [x.expected for x in rows]
    k_obs = [int(round(x.pvalue * S)) for x in rows]
    ones = np.ones(R, dtype=np.uint8)
    levels8 = [int(p * S) for p in (0.001, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5)]
    ptr = ctx.alloc(m.nbytes)
    t_up = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.h2d(ptr, m)
        t_up.append(time.perf_counter() - t0)
    ctx.set_kernel_times(True)
    plain = _timed(ctx, reps, ptr, R, S, ones, means, k_obs, [])
    with8 = _timed(ctx, reps, ptr, R, S, ones, means, k_obs, levels8)
    ctx.options["GAT_EFDR_LDS_THRESHOLDS"] = "64"
    chunked = _timed(ctx, reps, ptr, R, S, ones, means, k_obs, [])
    ctx.options.pop("GAT_EFDR_LDS_THRESHOLDS")
    assert np.array_equal(plain[3], with8[3]) and np.array_equal(plain[3], chunked[3])
    n_thr = len(set(k_obs))
    # the subsample's family on the device against the model (its rows are the first of the matrix: the same pointer)
    n_numpy = min(n_numpy, R)
    t0 = time.perf_counter()
    sub_k = E.k_obs_of(m[:n_numpy], means[:n_numpy], observed[:n_numpy])
    sub_v = E.counts(m[:n_numpy], means[:n_numpy], sub_k)
    E.adjusted(sub_k, sub_v, S)
    t_np = time.perf_counter() - t0
    assert sub_k == k_obs[:n_numpy]
    got_v, got_per = ctx.efdr_counts(ptr, n_numpy, S, ones[:n_numpy], means[:n_numpy], sub_k, levels8[:2])
    assert got_v.tolist() == sub_v, "device and model disagree"
    assert got_per.tolist() == E.per_sample(m[:n_numpy], means[:n_numpy], levels8[:2]).tolist(), "device and model disagree"
    # rows of three distinct values: every sample of a row in one of at most six bins
    tied = rs.choice([300.0, 301.0, 305.0], (R, S))
    ctx.h2d(ptr, tied)
    tied_means = [float(np.mean(r)) for r in tied]
    tied_k = E.k_obs_of(tied[:, :], tied_means, rs.choice([300.0, 301.0, 305.0], R))
    ties = _timed(ctx, reps, ptr, R, S, ones, tied_means, tied_k, [])
    ctx.set_kernel_times(False)
    ctx.free(ptr)
    t0 = time.perf_counter()
    minp._rows(rows)
    t_stack = time.perf_counter() - t0
    t0 = time.perf_counter()
    q, summary = efdr.compute(rows, [0.05, 0.2], ctx=ctx)
    t_all = time.perf_counter() - t0
    assert q == efdr.adjusted(k_obs, plain[3], S) and len(summary) == 6
    up = _median(t_up)
    gb = m.nbytes / 1e9
    scaled = t_np * R * R / (n_numpy * n_numpy)                          # (the model's K <= t comparisons grow with rows x thresholds)
    ms = lambda t: tuple(1e3 * x for x in t)  # noqa: E731
    moved = R * S * 12 / 1e9
    return [
        "%d rows x %d samples (%.2f GB of float64), %d distinct thresholds, medians of %d (lowest .. highest):" % (R, S, gb, n_thr, reps),
        "    upload of the matrix                     %9.2f ms  (%.2f .. %.2f)   %.1f GB/s" % (ms(up) + (gb / up[0],)),
        "    gat_efdr_counts, matrix on the device    %9.2f ms  (%.2f .. %.2f)" % ms(plain[0]),
        "        k_minp_rank (device time)            %9.2f ms  (%.2f .. %.2f)" % ms(plain[1]),
        "        k_efdr (device time), no level       %9.2f ms  (%.2f .. %.2f)   %.2f GB of K and matrix: %.0f GB/s"
        % (ms(plain[2]) + (moved, moved / plain[2][0] if plain[2][0] > 0 else 0.0)),
        "        k_efdr, 8 levels                     %9.2f ms  (%.2f .. %.2f)" % ms(with8[2]),
        "        k_efdr, chunks of 64 thresholds      %9.2f ms  (%.2f .. %.2f)   %d passes" % (ms(chunked[2]) + ((n_thr + 63) // 64,)),
        "        k_efdr, rows of three distinct values%9.2f ms  (%.2f .. %.2f)   %d distinct thresholds" % (ms(ties[2]) + (len(set(tied_k)),)),
        "    efdr.compute end to end, two cutoffs     %9.2f ms   of it on the host, k_obs and stacking the rows' samples: %.2f ms"
        % (1e3 * t_all, 1e3 * t_stack),
        "    numpy model (tests/efdr_model.py), %d rows: %.1f ms; scaled by rows x thresholds to %d rows: %.2f s"
        % (n_numpy, 1e3 * t_np, R, scaled),
        "    numpy / efdr.compute = %.1f;  of efdr.compute the upload is %.0f %%, the two kernels %.0f %%, the host's stacking %.0f %%;"
        " counts equal the model's on the %d rows"
        % (scaled / t_all, 100.0 * up[0] / t_all, 100.0 * (with8[1][0] + with8[2][0]) / t_all, 100.0 * t_stack / t_all, n_numpy),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--samples", default="10000,100000")
    ap.add_argument("--numpy-rows", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_efdr.txt"))
    a = ap.parse_args()
    rs = np.random.RandomState(2026)
    ctx = gat_amd.get_context()
    lines = ["resampling-based FDR (--qvalue-method=efdr, --output-stats=fdr_summary), MI355X, one GPU",
             "    python tools/time_efdr.py --rows %d --samples %s --numpy-rows %d --reps %d" % (a.rows, a.samples, a.numpy_rows, a.reps)]
    for S in [int(x) for x in a.samples.split(",")]:
        lines += shape(ctx, a.rows, S, a.numpy_rows, a.reps, rs)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
