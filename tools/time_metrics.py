#!/usr/bin/env python
"""Time gat_sample_metrics on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace
segment per contig), SamplerAnnotator:

  (a) the call end to end (wall clock around Problem.sample_metrics: sampler, k_metrics, the copy of the words),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone, so (a) - (b) is what the metrics cost,
  (c) the host route it replaces: Problem.sample (every list copied to the host) and numpy over the lists (searchsorted on
      the pieces' starts and ends, the sums of tests/metrics_model.words), on --host-samples samples, scaled,
  (d) the host time to format the rows: gat_amd.metrics.write_rows over --rows / 10 samples' words (ten rows a sample).

Medians over the repeats; the first call warms up.  The words of (a) and (c) over the host route's samples are compared on
the way.

    python tools/time_metrics.py [--samples 10000] [--host-samples 500] [--reps 3] [--rows 100000] [--out profiles/r14_metrics.txt]
"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gat_amd import _lib, metrics, problem, synthetic     # noqa: E402


def host_words(a, ws):
    """the eight sums of one list against normalized pieces, vectorised over the list's segments"""
    s, e = a["start"].astype(np.int64), a["end"].astype(np.int64)
    ws_s, ws_e = ws["start"].astype(np.int64), ws["end"].astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(ws_e - ws_s)])
    gaps = np.concatenate([[0], np.cumsum(ws_s[1:] > ws_e[:-1])]) if len(ws) else np.zeros(1, dtype=np.int64)
    lo = np.searchsorted(ws_e, s, side="right")
    hi = np.searchsorted(ws_s, e, side="left") - 1
    k = np.maximum(0, hi - lo + 1)
    t = k > 0
    lo_t, hi_t, s_t, e_t = lo[t], hi[t], s[t], e[t]
    inter = (cum[hi_t + 1] - cum[lo_t] - np.maximum(0, s_t - ws_s[lo_t]) - np.maximum(0, ws_e[hi_t] - e_t)).sum() if t.any() else 0
    pieces = int((~t).sum())
    if t.any():
        pieces += int((s_t < ws_s[lo_t]).sum() + (e_t > ws_e[hi_t]).sum() + (gaps[hi_t] - gaps[lo_t]).sum())
    last = int(s_t.max()) if t.any() else -1
    tail = s > last
    return [len(a), int((e - s).sum()), int(k.sum()), int(inter), int((e_t - s_t).sum()), pieces, int(tail.sum()), int((e - s)[tail].sum())]


def host_route(P, seed, n_samples, ws, ws_off):
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    out = np.zeros((n_samples, C, len(metrics.WORDS)), dtype=np.int64)
    for i in range(n_samples):
        for c in range(C):
            out[i, c] = host_words(seg[off[i * C + c]:off[i * C + c + 1]], ws[ws_off[c]:ws_off[c + 1]])
    return out, len(seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_metrics.txt"))
    a = ap.parse_args()
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    per = [cfg["workspace"][c] for c in flat["contig_names"]]
    ws = np.concatenate(per)
    ws_off = np.concatenate([[0], np.cumsum([len(w) for w in per])]).astype(np.int64)
    size = np.array([int((w["end"].astype(np.int64) - w["start"]).sum()) for w in per], dtype=np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_metrics.py --samples %d --host-samples %d --reps %d --rows %d" % (a.samples, a.host_samples, a.reps, a.rows),
             "gat_sample_metrics on the config-2 geometry: %d units, %d segments, %d workspace pieces, SamplerAnnotator, %d samples, "
             "MI355X, one GPU" % (flat["n_units"], len(flat["segs"]), len(ws), a.samples)]
    wall, sampler = [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        got = P.sample_metrics(7, 0, a.samples, ws, ws_off)
        wall.append((time.perf_counter() - t0) * 1e3)
        sampler.append(P.last_stats["ms_sampler"])
    batches = P.last_stats["n_batches"]
    wall, sampler = sorted(wall[1:]), sorted(sampler[1:])
    ms_a, ms_b = wall[len(wall) // 2], sampler[len(sampler) // 2]
    t0 = time.perf_counter()
    host, n_seg = host_route(P, 7, a.host_samples, ws, ws_off)
    ms_host = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    P.sample(7, 0, a.host_samples)
    ms_copy = (time.perf_counter() - t0) * 1e3
    same = np.array_equal(host, got[:a.host_samples])
    ms_c = ms_host * a.samples / a.host_samples
    n_fmt = max(1, a.rows // len(metrics.ATTRIBUTES))
    words = np.concatenate([got] * (n_fmt // len(got) + 1))[:n_fmt]
    fmt = []
    for r in range(a.reps):
        sink = io.StringIO()
        t0 = time.perf_counter()
        metrics.write_rows(sink, "merged", [str(i) for i in range(n_fmt)], words, size)
        fmt.append((time.perf_counter() - t0) * 1e3)
    n_rows = sink.getvalue().count("\n")
    fmt.sort()
    lines += [
        "%d lists of %.0f segments on average, %d batches; sampled bases %d, of them inside the workspace %d" % (
            got.shape[0] * got.shape[1], got[:, :, 0].mean(), batches, int(got[:, :, 1].sum()), int(got[:, :, 3].sum())),
        "    (a) gat_sample_metrics end to end                 %9.1f ms  (%.1f .. %.1f)" % (ms_a, wall[0], wall[-1]),
        "    (b) ms_sampler of the same call                   %9.1f ms  (%.1f .. %.1f)" % (ms_b, sampler[0], sampler[-1]),
        "        (a) - (b): k_metrics and the copy of the words %8.1f ms" % (ms_a - ms_b),
        "    (c) Problem.sample + numpy, %d samples: %.1f ms (%d segments; the copy-out alone %.1f ms), scaled to %d samples %9.1f ms" % (
            a.host_samples, ms_host, n_seg, ms_copy, a.samples, ms_c),
        "        (c) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_c / ms_a, a.host_samples,
                                                                                        "equal" if same else "DIFFERENT"),
        "    (d) formatting %d rows on the host (metrics.write_rows, %d values a row) %9.1f ms  (%.1f .. %.1f)" % (
            n_rows, got.shape[1], fmt[len(fmt) // 2], fmt[0], fmt[-1]),
    ]
    P.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
