#!/usr/bin/env python
"""Time --qvalue-method=minp (step-down minP, gat_amd/minp.py) on synthetic count matrices: per shape the upload of the
float64 matrix, gat_minp_counts on the resident matrix (host clock around the synchronous call) with the device time of
k_minp_rank and k_minp_step separately (events, gat_minp_times), the same with every digit pass of the sort run
(GAT_MINP_ALL_PASSES: what skipping the digits in which all keys agree is worth), the whole minp.adjust call (k_obs and stacking the
rows on the host, upload, device, running maximum), and the numpy model of tests/minp_model.py -- vectorised over samples -- on a
subsample of the rows, scaled to all of them.  The counts of the subsample's family are checked against the model.

    python tools/time_minp.py [--rows 1000] [--samples 10000,100000] [--numpy-rows 40] [--reps 3] [--out FILE]
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
import minp_model as M                           # noqa: E402
from gat_amd import minp                         # noqa: E402


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def shape(ctx, R, S, n_numpy, reps, rs):
    # counts of a run: per annotation a level and Poisson scatter around it; the observed value near the level
    level = rs.randint(200, 20000, R)
    m = rs.poisson(level[:, None], (R, S)).astype(np.float64)
    observed = np.maximum(1, (level * rs.uniform(0.97, 1.03, R)).astype(np.int64)).astype(np.float64)
    rows = [gat_amd.AnnotatorResult("merged", "a%04d" % i, "na", o, r) for i, (o, r) in enumerate(zip(observed, m))]
    means = [x.expected for x in rows]
    k_obs = [int(round(x.pvalue * S)) for x in rows]
    ones = np.ones(R, dtype=np.uint8)
    ptr = ctx.alloc(m.nbytes)
    t_up = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.h2d(ptr, m)
        t_up.append(time.perf_counter() - t0)
    ctx.set_kernel_times(True)
    timings = {}
    for tag, all_passes in (("skip", None), ("all", "1")):
        if all_passes:
            ctx.options["GAT_MINP_ALL_PASSES"] = all_passes
        t_call, t_rank, t_step = [], [], []
        for _ in range(reps + 1):                                        # (the first call warms up: not counted)
            t0 = time.perf_counter()
            c = ctx.minp_counts(ptr, R, S, ones, means, k_obs)
            t_call.append(time.perf_counter() - t0)
            a, b = ctx.minp_times()
            t_rank.append(a * 1e-3)
            t_step.append(b * 1e-3)
        timings[tag] = (_median(t_call[1:]), _median(t_rank[1:]), _median(t_step[1:]), c.copy())
        if all_passes:
            ctx.options.pop("GAT_MINP_ALL_PASSES")
    ctx.set_kernel_times(False)
    assert np.array_equal(timings["skip"][3], timings["all"][3])
    # the subsample's family on the device against the model (its rows are the first of the matrix: the same pointer)
    n_numpy = min(n_numpy, R)
    t0 = time.perf_counter()
    sub_k = M.k_obs_of(m[:n_numpy], means[:n_numpy], observed[:n_numpy])
    sub_c = M.counts(m[:n_numpy], means[:n_numpy], sub_k)
    M.adjusted(sub_k, sub_c, S)
    t_np = time.perf_counter() - t0
    assert sub_k == k_obs[:n_numpy]
    got = ctx.minp_counts(ptr, n_numpy, S, ones[:n_numpy], means[:n_numpy], sub_k).tolist()
    assert got == sub_c, "device and model disagree"
    ctx.free(ptr)
    t0 = time.perf_counter()
    minp._rows(rows)
    t_stack = time.perf_counter() - t0
    t0 = time.perf_counter()
    adj = minp.adjust(rows, ctx=ctx)
    t_all = time.perf_counter() - t0
    assert adj == minp.adjusted(k_obs, timings["skip"][3], S)
    (call, rank, step, _), (call_a, rank_a, _, _) = timings["skip"], timings["all"]
    up = _median(t_up)
    gb = m.nbytes / 1e9
    scaled = t_np * R / n_numpy
    ms = lambda t: tuple(1e3 * x for x in t)  # noqa: E731
    return [
        "%d rows x %d samples (%.2f GB of float64), medians of %d (lowest .. highest):" % (R, S, gb, reps),
        "    upload of the matrix                     %9.2f ms  (%.2f .. %.2f)   %.1f GB/s" % (ms(up) + (gb / up[0],)),
        "    gat_minp_counts, matrix on the device    %9.2f ms  (%.2f .. %.2f)" % ms(call),
        "        k_minp_rank (device time)            %9.2f ms  (%.2f .. %.2f)" % ms(rank),
        "        k_minp_step (device time)            %9.2f ms  (%.2f .. %.2f)" % ms(step),
        "    ... with all 16 digit passes             %9.2f ms  (%.2f .. %.2f)   k_minp_rank %.2f ms: the skip saves %.0f %% of the kernel"
        % (ms(call_a) + (1e3 * rank_a[0], 100.0 * (1.0 - rank[0] / rank_a[0]) if rank_a[0] > 0 else 0.0)),
        "    minp.adjust end to end (one call)        %9.2f ms   of it on the host, k_obs and stacking the rows' samples: %.2f ms"
        % (1e3 * t_all, 1e3 * t_stack),
        "    numpy model (tests/minp_model.py, vectorised over samples), %d rows: %.1f ms; scaled to %d rows: %.2f s"
        % (n_numpy, 1e3 * t_np, R, scaled),
        "    numpy / minp.adjust = %.1f;  of minp.adjust the upload is %.0f %%, the two kernels %.0f %%, the host's stacking %.0f %%;"
        " counts equal the model's on the %d rows"
        % (scaled / t_all, 100.0 * up[0] / t_all, 100.0 * (rank[0] + step[0]) / t_all, 100.0 * t_stack / t_all, n_numpy),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--samples", default="10000,100000")
    ap.add_argument("--numpy-rows", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_minp.txt"))
    a = ap.parse_args()
    rs = np.random.RandomState(2026)
    ctx = gat_amd.get_context()
    lines = ["step-down minP (--qvalue-method=minp), MI355X, one GPU",
             "    python tools/time_minp.py --rows %d --samples %s --numpy-rows %d --reps %d" % (a.rows, a.samples, a.numpy_rows, a.reps)]
    for S in [int(x) for x in a.samples.split(",")]:
        lines += shape(ctx, a.rows, S, a.numpy_rows, a.reps, rs)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
