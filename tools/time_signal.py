#!/usr/bin/env python
"""Time gat_sample_signal on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace segment
per contig), SamplerAnnotator, in two cases: ONE genome-wide signal track of 1 kb pieces (some 3.1 million pieces, every base
carries a value), and TEN tracks of 100 kb pieces.  Per case:

  (a) the call end to end (wall clock around Problem.sample_signal: sampler, k_signal, the copy of the words),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone, so (a) - (b) is what the signal costs,
  (d) gat_sample_distances, direction 0, on the same lists against the same piece intervals: k_distance makes the same first
      search per segment, and (a) - (b) of that call is the yardstick,
  (c) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists (prefix sums and two
      searchsorted per pair of lists, the definition of include/gat_mi355.h), on --host-samples samples, scaled.
  (e) the part of (a) that does not depend on the samples: gat_list_signal of one list of one segment against the same tracks
      -- the host's checks, the records built and uploaded -- so (a) - (b) - (e) is k_signal and the copy of the words,

and (b) is the sampler stage as it was before the call existed (its code is the same): the yardstick the numbers are recorded
next to.  Medians over the repeats; the first call warms up.  The words of (a) and (c) over the host route's samples are
compared on the way.  No threshold: the numbers are recorded.

    python tools/time_signal.py [--samples 10000] [--host-samples 100] [--reps 3] [--out profiles/r24_signal.txt]
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


def tiled_track(contigs, piece, seed, lo=-2000, hi=2000):
    """per contig: pieces of `piece` bases over its whole length (the last one short), values uniform in [lo, hi]"""
    rs = np.random.RandomState(seed)
    per = []
    for c in contigs:
        start = np.arange(0, synthetic.HG19[c], piece, dtype=np.int64)
        end = np.minimum(start + piece, synthetic.HG19[c])
        per.append((intervals.make(start, end), rs.randint(lo, hi + 1, size=len(start)).astype(np.int32)))
    return per


def host_words(q, pieces, values, pc, pw):
    """the four sums of the segments q against one contig's pieces, vectorised over the segments (pc, pw: the prefix sums)"""
    qs, qe = q["start"].astype(np.int64), q["end"].astype(np.int64)
    keep = qe > qs
    qs, qe = qs[keep], qe[keep]
    K = len(pieces)
    if K == 0 or len(qs) == 0:
        return [len(qs), 0, 0, 0]
    ps, pe = pieces["start"].astype(np.int64), pieces["end"].astype(np.int64)
    j0 = np.searchsorted(pe, qs, side="right")
    j1 = np.searchsorted(pe, qe, side="left")
    last = np.where((j1 < K) & (ps[np.minimum(j1, K - 1)] < qe), j1, j1 - 1)
    hit = j0 <= last
    a, b = np.minimum(j0, K - 1), np.clip(last, 0, K - 1)
    c = pc[b + 1] - pc[a] - np.maximum(qs - ps[a], 0) - np.maximum(pe[b] - qe, 0)
    w = pw[b + 1] - pw[a] - values[a] * np.maximum(qs - ps[a], 0) - values[b] * np.maximum(pe[b] - qe, 0)
    return [len(qs), int(c[hit].sum()), int(hit.sum()), int(w[hit].sum())]


def host_route(P, seed, n_samples, tracks):
    """tracks[t][c] = (pieces, values).  Returns (int64 [n_samples, n_tracks, 4], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    prefix = [[(np.concatenate([[0], np.cumsum(p["end"].astype(np.int64) - p["start"].astype(np.int64))]),
                np.concatenate([[0], np.cumsum(v.astype(np.int64) * (p["end"].astype(np.int64) - p["start"].astype(np.int64)))]))
               for p, v in per] for per in tracks]
    out = np.zeros((n_samples, len(tracks), 4), dtype=np.int64)
    for i in range(n_samples):
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            for t, per in enumerate(tracks):
                out[i, t] += host_words(a, per[c][0], per[c][1].astype(np.int64), *prefix[t][c])
    return out, len(seg)


def median(x):
    x = sorted(x)
    return x[len(x) // 2], x[0], x[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_signal.txt"))
    a = ap.parse_args()
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_signal.py --samples %d --host-samples %d --reps %d" % (a.samples, a.host_samples, a.reps),
             "gat_sample_signal on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, MI355X, one GPU" % (
                 flat["n_units"], len(flat["segs"]), a.samples)]
    for name, n_tracks, piece in (("one genome-wide track of 1 kb pieces", 1, 1000), ("ten tracks of 100 kb pieces", 10, 100000)):
        tracks = [tiled_track(contigs, piece, 300 + t) for t in range(n_tracks)]
        flat_lists = [x for per in tracks for x in per]
        pieces = np.concatenate([p for p, _ in flat_lists])
        values = np.concatenate([v for _, v in flat_lists])
        piece_off = np.concatenate([[0], np.cumsum([len(p) for p, _ in flat_lists])]).astype(np.int64)
        wall, sampler, d_wall, d_sampler = [], [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_signal(7, 0, a.samples, pieces, values, piece_off, n_tracks)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
        batches = P.last_stats["n_batches"]
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            dist = P.sample_distances(7, 0, a.samples, pieces, piece_off, n_tracks, 0, MAX_DISTANCE)
            d_wall.append((time.perf_counter() - t0) * 1e3)
            d_sampler.append(P.last_stats["ms_sampler"])
        one = np.zeros(1, dtype=_lib.SEG)
        one["start"], one["end"] = 1000, 1400
        one_off = np.concatenate([[0], np.ones(len(contigs), dtype=np.int64)])
        fixed = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            _lib.list_signal(ctx, one, one_off, 1, pieces, values, piece_off, n_tracks, len(contigs))
            fixed.append((time.perf_counter() - t0) * 1e3)
        ms_e, e_lo, e_hi = median(fixed[1:])
        (ms_a, a_lo, a_hi), (ms_b, b_lo, b_hi) = median(wall[1:]), median(sampler[1:])
        (ms_d, d_lo, d_hi), (ms_ds, _, _) = median(d_wall[1:]), median(d_sampler[1:])
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, tracks)
        ms_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        P.sample(7, 0, a.host_samples)
        ms_copy = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, got[:a.host_samples])
        ms_c = ms_host * a.samples / a.host_samples
        lines += [
            "%s: %d pieces in all, %d (segment, track) pairs counted, %d of them hit, %d of the distances' queries within %d; %d batches" % (
                name, len(pieces), int(got[:, :, 0].sum()), int(got[:, :, 2].sum()), int(dist[:, :, 2].sum()), MAX_DISTANCE, batches),
            "    (a) gat_sample_signal end to end                    %9.1f ms  (%.1f .. %.1f)" % (ms_a, a_lo, a_hi),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, b_lo, b_hi),
            "        (a) - (b): the records, k_signal and the copy of the words %9.1f ms" % (ms_a - ms_b),
            "    (e) gat_list_signal of one segment, same tracks (checks, records built and uploaded) %9.1f ms  (%.1f .. %.1f)" % (ms_e, e_lo, e_hi),
            "        (a) - (b) - (e): k_signal and the copy of the words %9.1f ms" % (ms_a - ms_b - ms_e),
            "    (d) gat_sample_distances, direction 0, same lists and piece intervals: %9.1f ms  (%.1f .. %.1f), ms_sampler %.1f ms, "
            "k_distance and its copies %.1f ms" % (ms_d, d_lo, d_hi, ms_ds, ms_d - ms_ds),
            "        ((a) - (b) - (e)) / (d's difference) = %.2f" % ((ms_a - ms_b - ms_e) / max(1e-9, ms_d - ms_ds)),
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
