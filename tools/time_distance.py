#!/usr/bin/env python
"""Time gat_sample_distances on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace
segment per contig), SamplerAnnotator, against --tracks synthetic annotation tracks of --intervals intervals each, in both
directions:

  (a) the call end to end (wall clock around Problem.sample_distances: sampler, k_distance, the copy of the words),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone, so (a) - (b) is what the distances cost,
  (c) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists (one searchsorted on
      the ends per pair of lists, the definition of include/gat_mi355.h), on --host-samples samples, scaled.

Medians over the repeats; the first call warms up.  The words of (a) and (c) over the host route's samples are compared on
the way.

    python tools/time_distance.py [--samples 10000] [--host-samples 200] [--tracks 10] [--intervals 2000] [--reps 3]
                                  [--out profiles/r15_distance.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gat_amd import _lib, intervals, problem, synthetic     # noqa: E402

MAX_DISTANCE = 1000


def host_words(q, t, max_distance):
    """the four sums of the queries q against the normalized list t, vectorised over the queries"""
    qs, qe = q["start"].astype(np.int64), q["end"].astype(np.int64)
    keep = qe > qs
    qs, qe = qs[keep], qe[keep]
    K = len(t)
    if K == 0:
        return [0, 0, 0, len(qs)]
    ts, te = t["start"].astype(np.int64), t["end"].astype(np.int64)
    j = np.searchsorted(te, qs, side="right")
    big = np.int64(1) << 40
    nxt = ts[np.minimum(j, K - 1)]
    right = np.where(j < K, nxt - qe + 1, big)
    left = np.where(j > 0, qs - te[np.maximum(j, 1) - 1] + 1, big)
    d = np.where((j < K) & (nxt < qe), 0, np.minimum(left, right))
    return [len(qs), int(d.sum()), int((d <= max_distance).sum()), 0]


def host_route(P, seed, n_samples, tracks, direction):
    """tracks[t][c]: SEG arrays.  Returns (int64 [n_samples, n_tracks, 4], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    out = np.zeros((n_samples, len(tracks), 4), dtype=np.int64)
    for i in range(n_samples):
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            for t, per in enumerate(tracks):
                out[i, t] += host_words(a, per[c], MAX_DISTANCE) if direction == 0 else host_words(per[c], a, MAX_DISTANCE)
    return out, len(seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=200)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--intervals", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_distance.txt"))
    a = ap.parse_args()
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
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_distance.py --samples %d --host-samples %d --tracks %d --intervals %d --reps %d" % (
                 a.samples, a.host_samples, a.tracks, a.intervals, a.reps),
             "gat_sample_distances on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, %d annotation tracks "
             "of %d intervals in all, max_distance %d, MI355X, one GPU" % (flat["n_units"], len(flat["segs"]), a.samples, a.tracks,
                                                                            len(annos), MAX_DISTANCE)]
    for direction, name in ((0, "segment to annotation"), (1, "annotation to segment")):
        wall, sampler = [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_distances(7, 0, a.samples, annos, anno_off, a.tracks, direction, MAX_DISTANCE)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
        batches = P.last_stats["n_batches"]
        wall, sampler = sorted(wall[1:]), sorted(sampler[1:])
        ms_a, ms_b = wall[len(wall) // 2], sampler[len(sampler) // 2]
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, tracks, direction)
        ms_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        P.sample(7, 0, a.host_samples)
        ms_copy = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, got[:a.host_samples])
        ms_c = ms_host * a.samples / a.host_samples
        lines += [
            "direction %d, %s: %d queries counted, %d of them within %d, %d without a neighbour on their contig; %d batches" % (
                direction, name, int(got[:, :, 0].sum()), int(got[:, :, 2].sum()), MAX_DISTANCE, int(got[:, :, 3].sum()), batches),
            "    (a) gat_sample_distances end to end                 %9.1f ms  (%.1f .. %.1f)" % (ms_a, wall[0], wall[-1]),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, sampler[0], sampler[-1]),
            "        (a) - (b): k_distance and the copy of the words %9.1f ms" % (ms_a - ms_b),
            "    (c) Problem.sample + numpy, %d samples: %.1f ms (%d segments; the copy-out alone %.1f ms), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, ms_copy, a.samples, ms_c),
            "        (c) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_c / ms_a, a.host_samples,
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
