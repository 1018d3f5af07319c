#!/usr/bin/env python
"""Time gat_sample_coverage on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace
segment per contig), SamplerAnnotator, at bin sizes 1 000 and 100 000:

  (a) the call end to end (wall clock around Problem.sample_coverage: sampler, k_coverage, the copy of the sums),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone, so (a) - (b) is what the coverage costs,
  (c) the host route it replaces: Problem.sample (every list copied to the host) and numpy over the lists
      (gat_amd.coverage.bin_bases for the bases, bincount for the starts and ends), on --host-samples samples, scaled.

Medians over the repeats; the first call of each bin size warms up.  The sums of (a) and (c) over the host route's samples
are compared on the way.

    python tools/time_coverage.py [--samples 10000] [--host-samples 500] [--reps 3] [--out profiles/r13_coverage.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gat_amd import _lib, coverage, problem, synthetic     # noqa: E402


def host_route(P, seed, n_samples, bin_size, n_bins):
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    bases, starts, ends = [], [], []
    for c in range(C):
        lists = np.concatenate([seg[off[i * C + c]:off[i * C + c + 1]] for i in range(n_samples)])
        bases.append(coverage.bin_bases(lists, bin_size, int(n_bins[c])))
        s, e = lists["start"].astype(np.int64) // bin_size, (lists["end"].astype(np.int64) - 1) // bin_size
        starts.append(np.bincount(s[s < n_bins[c]], minlength=int(n_bins[c])))
        ends.append(np.bincount(e[e < n_bins[c]], minlength=int(n_bins[c])))
    return np.concatenate(bases), np.concatenate(starts), np.concatenate(ends), len(seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_coverage.txt"))
    a = ap.parse_args()
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    ext = np.array([int(cfg["workspace"][c]["end"].max()) for c in flat["contig_names"]], dtype=np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["gat_sample_coverage on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, MI355X, one GPU"
             % (flat["n_units"], len(flat["segs"]), a.samples),
             "    python tools/time_coverage.py --samples %d --host-samples %d --reps %d" % (a.samples, a.host_samples, a.reps)]
    for bin_size in (1000, 100000):
        n_bins = (ext + bin_size - 1) // bin_size
        wall, sampler = [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_coverage(7, 0, a.samples, bin_size, n_bins)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
        batches = P.last_stats["n_batches"]
        wall, sampler = sorted(wall[1:]), sorted(sampler[1:])
        ms_a, ms_b = wall[len(wall) // 2], sampler[len(sampler) // 2]
        small = P.sample_coverage(7, 0, a.host_samples, bin_size, n_bins)
        t0 = time.perf_counter()
        hb, hs, he, n_seg = host_route(P, 7, a.host_samples, bin_size, n_bins)
        ms_host = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(hb, small[0]) and np.array_equal(hs, small[1]) and np.array_equal(he, small[2])
        ms_c = ms_host * a.samples / a.host_samples
        lines += [
            "bin size %d: %d bins, %d batches; sampled bases %d, beyond the last bin %d" % (bin_size, int(n_bins.sum()), batches,
                                                                                          int(got[0].sum()), int(got[3].sum())),
            "    (a) gat_sample_coverage end to end              %9.1f ms  (%.1f .. %.1f)" % (ms_a, wall[0], wall[-1]),
            "    (b) ms_sampler of the same call                 %9.1f ms  (%.1f .. %.1f)" % (ms_b, sampler[0], sampler[-1]),
            "        (a) - (b): k_coverage and the copy of the sums %6.1f ms" % (ms_a - ms_b),
            "    (c) Problem.sample + numpy, %d samples: %.1f ms (%d segments), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, a.samples, ms_c),
            "        (c) / (a) = %.1f; the two routes' sums over those %d samples are %s" % (ms_c / ms_a, a.host_samples,
                                                                                          "equal" if same else "DIFFERENT"),
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
