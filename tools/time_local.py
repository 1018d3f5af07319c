#!/usr/bin/env python
"""Time gat_sample_bin_enrichment on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace
segment per contig), SamplerAnnotator, against --tracks synthetic annotation tracks of --intervals intervals each, at every
--bin-size:

  (a) the call end to end (wall clock around Problem.sample_bin_enrichment: the windows made on the host, obs up, the sampler,
      k_local behind every batch, k_null_finish, the five words per (track, bin) down),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone,
  (c) the same call over ONE sample -- the fixed cost of a call (windows, obs up, words down), so (a) - (b) - (c) is close to
      what k_local costs over the samples,
  (d) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists -- the pieces of list
      n track cut at the bin edges and added into the five words -- on --host-samples samples, scaled.

Medians over the repeats; the first call warms up.  The words of (a)'s route and (d) over the host route's samples are compared
on the way.

    python tools/time_local.py [--samples 10000] [--host-samples 20] [--tracks 10] [--intervals 2000] [--reps 3]
                               [--bin-size 1000 --bin-size 100000] [--out profiles/r18_local.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gat_amd import _lib, intervals, problem, synthetic     # noqa: E402


def pieces_of(a, t):
    """the pieces of a n t, both normalized SEG arrays: int64 starts, ends"""
    if len(a) == 0 or len(t) == 0:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    cuts = np.unique(np.concatenate([a["start"], a["end"], t["start"], t["end"]]).astype(np.int64))
    lo, hi = cuts[:-1], cuts[1:]

    def inside(x):                                      # the elementary interval [lo, hi) lies in an interval of x
        k = np.searchsorted(x["start"].astype(np.int64), lo, side="right") - 1
        return (k >= 0) & (x["end"].astype(np.int64)[np.maximum(k, 0)] >= hi)

    keep = inside(a) & inside(t)
    return lo[keep], hi[keep]


def bin_values(s, e, bin_size, n_bins):
    """(bins, values) of disjoint pieces: the pieces cut at the bin edges, the parts summed per bin; bins ascending"""
    keep = s < n_bins * bin_size
    s, e = s[keep], np.minimum(e[keep], n_bins * bin_size)
    fb, lb = s // bin_size, (e - 1) // bin_size
    reps = lb - fb + 1
    first = np.repeat(np.cumsum(reps) - reps, reps)
    b = np.repeat(fb, reps) + (np.arange(int(reps.sum())) - first)
    ps, pe = np.maximum(np.repeat(s, reps), b * bin_size), np.minimum(np.repeat(e, reps), (b + 1) * bin_size)
    bins, inv = np.unique(b, return_inverse=True)
    return bins, np.bincount(inv, weights=(pe - ps).astype(np.float64), minlength=len(bins)).astype(np.int64)


def host_route(P, seed, n_samples, tracks, bin_size, n_bins, bin_off, obs):
    """tracks[t][c]: SEG arrays.  Returns (int64 [n_tracks, total_bins, 5], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    out = np.zeros((len(tracks), int(bin_off[-1]), 5), dtype=np.int64)
    for i in range(n_samples):
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            for t, per in enumerate(tracks):
                bins, v = bin_values(*pieces_of(a, per[c]), bin_size, int(n_bins[c]))
                k = bins + int(bin_off[c])
                o = obs[t, k]
                out[t, k, 0] += 1
                out[t, k, 1] += v
                out[t, k, 2] += v * v
                out[t, k, 3] += v < o
                out[t, k, 4] += v == o
    zeros = n_samples - out[..., 0]
    out[..., 3] += zeros * (obs > 0)
    out[..., 4] += zeros * (obs == 0)
    return out, len(seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=20)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--intervals", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bin-size", type=int, action="append")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_local.txt"))
    a = ap.parse_args()
    bin_sizes = a.bin_size or [1000, 100000]
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    tracks = []
    for t in range(a.tracks):
        per = synthetic.random_segments(synthetic.HG19, a.intervals, 300, 200 + t)
        tracks.append([intervals.normalize(per[c]) if c in per else intervals.EMPTY for c in contigs])
    lists = [x for per in tracks for x in per]
    annos = np.concatenate(lists)
    anno_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    segs = [intervals.normalize(cfg["segments"][c]) if c in cfg["segments"] else intervals.EMPTY for c in contigs]
    seg_all = np.concatenate(segs)
    seg_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_local.py --samples %d --host-samples %d --tracks %d --intervals %d --reps %d %s" % (
                 a.samples, a.host_samples, a.tracks, a.intervals, a.reps, " ".join("--bin-size %d" % b for b in bin_sizes)),
             "gat_sample_bin_enrichment on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, %d annotation "
             "tracks of %d intervals in all, MI355X, one GPU" % (flat["n_units"], len(flat["segs"]), a.samples, a.tracks, len(annos))]
    for bin_size in bin_sizes:
        n_bins = np.array([(int(cfg["workspace"][c]["end"].max()) + bin_size - 1) // bin_size for c in contigs], dtype=np.int64)
        t0 = time.perf_counter()
        observed, bin_off = ctx.list_bin_overlaps(seg_all, seg_off, 1, annos, anno_off, a.tracks, len(contigs), bin_size, n_bins)
        ms_obs = (time.perf_counter() - t0) * 1e3
        obs = observed[0]
        wall, sampler, fixed = [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got, _ = P.sample_bin_enrichment(7, 0, a.samples, annos, anno_off, a.tracks, bin_size, n_bins, obs)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
            batches = P.last_stats["n_batches"]
            t0 = time.perf_counter()
            P.sample_bin_enrichment(7, 0, 1, annos, anno_off, a.tracks, bin_size, n_bins, obs)
            fixed.append((time.perf_counter() - t0) * 1e3)
        wall, sampler, fixed = sorted(wall[1:]), sorted(sampler[1:]), sorted(fixed[1:])
        ms_a, ms_b, ms_c = wall[len(wall) // 2], sampler[len(sampler) // 2], fixed[len(fixed) // 2]
        part, _ = P.sample_bin_enrichment(7, 0, a.host_samples, annos, anno_off, a.tracks, bin_size, n_bins, obs)
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, tracks, bin_size, n_bins, bin_off, obs)
        ms_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        P.sample(7, 0, a.host_samples)
        ms_copy = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, part)
        ms_d = ms_host * a.samples / a.host_samples
        lines += [
            "bin_size %d: %d bins x %d tracks = %d (track, bin) pairs, %d of them reached by a sample, %d with an observed base "
            "(gat_list_bin_overlaps: %.1f ms); %d batches" % (bin_size, int(bin_off[-1]), a.tracks, int(bin_off[-1]) * a.tracks,
                                                              int((got[..., 0] > 0).sum()), int((obs > 0).sum()), ms_obs, batches),
            "    (a) gat_sample_bin_enrichment end to end            %9.1f ms  (%.1f .. %.1f)" % (ms_a, wall[0], wall[-1]),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, sampler[0], sampler[-1]),
            "    (c) the same call over one sample (windows, obs up, words down: %d MB) %9.1f ms  (%.1f .. %.1f)" % (
                got.nbytes >> 20, ms_c, fixed[0], fixed[-1]),
            "        (a) - (b) - (c): k_local over the samples       %9.1f ms = %.2f x the sampler" % (ms_a - ms_b - ms_c,
                                                                                                     (ms_a - ms_b - ms_c) / max(ms_b, 1e-9)),
            "    (d) Problem.sample + numpy, %d samples: %.1f ms (%d segments; the copy-out alone %.1f ms), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, ms_copy, a.samples, ms_d),
            "        (d) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_d / ms_a, a.host_samples,
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
