#!/usr/bin/env python
"""Time gat_sample_pair_enrichment on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace
segment per contig), SamplerAnnotator, against synthetic annotation tracks of --intervals intervals each, for every --tracks:

  (a) the call end to end (wall clock around Problem.sample_pair_enrichment: the tracks and obs up, the sampler, k_pairs behind
      every batch, k_null_finish, the five words per pair down),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone,
  (c) the same call over ONE sample -- the fixed cost of a call, so (a) - (b) - (c) is close to what k_pairs costs over the
      samples,
  (e) gat_sample_distances, direction 0, on the same tracks and samples, with its own (b) and (c): the same searches -- one per
      (segment, track) -- without the pair phase, so the ratio of the two kernels' times says what the pair phase costs,
  (d) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists -- a search per
      (list, track), the hit matrix times its transpose -- on --host-samples samples, scaled.

Medians over the repeats; the first call warms up.  The words of (a)'s route and (d) over the host route's samples are compared
on the way.

    python tools/time_pairs.py [--samples 10000] [--host-samples 20] [--tracks 10 --tracks 100] [--intervals 2000] [--reps 3]
                               [--out profiles/r19_pairs.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gat_amd import _lib, intervals, problem, synthetic     # noqa: E402


def hits(a, t):
    """per segment of a (any order), whether it shares a base with an interval of the normalized t"""
    if len(a) == 0 or len(t) == 0:
        return np.zeros(len(a), dtype=bool)
    s, e = a["start"].astype(np.int64), a["end"].astype(np.int64)
    j = np.searchsorted(t["end"].astype(np.int64), s, side="right")
    return (e > s) & (j < len(t)) & (t["start"].astype(np.int64)[np.minimum(j, len(t) - 1)] < e)


def host_route(P, seed, n_samples, tracks, obs):
    """tracks[t][c]: SEG arrays.  Returns (int64 [P, 5], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C, T = P.n_contigs, len(tracks)
    iu = np.triu_indices(T)
    out = np.zeros((len(iu[0]), 5), dtype=np.int64)
    for i in range(n_samples):
        full = np.zeros((T, T), dtype=np.int64)
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            h = np.stack([hits(a, per[c]) for per in tracks], axis=1).astype(np.int64)
            full += h.T @ h
        v = full[iu]
        out[:, 0] += v > 0
        out[:, 1] += v
        out[:, 2] += v * v
        out[:, 3] += v < obs
        out[:, 4] += v == obs
    return out, len(seg)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=20)
    ap.add_argument("--tracks", type=int, action="append")
    ap.add_argument("--intervals", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_pairs.txt"))
    a = ap.parse_args()
    n_tracks = a.tracks or [10, 100]
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    segs = [intervals.normalize(cfg["segments"][c]) if c in cfg["segments"] else intervals.EMPTY for c in contigs]
    seg_all = np.concatenate(segs)
    seg_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_pairs.py --samples %d --host-samples %d %s --intervals %d --reps %d" % (
                 a.samples, a.host_samples, " ".join("--tracks %d" % t for t in n_tracks), a.intervals, a.reps),
             "gat_sample_pair_enrichment on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, annotation "
             "tracks of %d intervals each, MI355X, one GPU" % (flat["n_units"], len(flat["segs"]), a.samples, a.intervals)]
    for T in n_tracks:
        tracks = []
        for t in range(T):
            per = synthetic.random_segments(synthetic.HG19, a.intervals, 300, 200 + t)
            tracks.append([intervals.normalize(per[c]) if c in per else intervals.EMPTY for c in contigs])
        lists = [x for per in tracks for x in per]
        annos = np.concatenate(lists)
        anno_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        t0 = time.perf_counter()
        obs = ctx.list_pair_hits(seg_all, seg_off, 1, annos, anno_off, T, len(contigs))[0]
        ms_obs = (time.perf_counter() - t0) * 1e3
        wall, sampler, fixed, d_wall, d_sampler, d_fixed = [], [], [], [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_pair_enrichment(7, 0, a.samples, annos, anno_off, T, obs)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
            batches = P.last_stats["n_batches"]
            t0 = time.perf_counter()
            P.sample_pair_enrichment(7, 0, 1, annos, anno_off, T, obs)
            fixed.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            P.sample_distances(7, 0, a.samples, annos, anno_off, T, 0, 0)
            d_wall.append((time.perf_counter() - t0) * 1e3)
            d_sampler.append(P.last_stats["ms_sampler"])
            t0 = time.perf_counter()
            P.sample_distances(7, 0, 1, annos, anno_off, T, 0, 0)
            d_fixed.append((time.perf_counter() - t0) * 1e3)
        (ms_a, a0, a1), (ms_b, b0, b1), (ms_c, c0, c1) = median(wall[1:]), median(sampler[1:]), median(fixed[1:])
        (ms_e, e0, e1), (ms_eb, _, _), (ms_ec, _, _) = median(d_wall[1:]), median(d_sampler[1:]), median(d_fixed[1:])
        k_pairs, k_distance = ms_a - ms_b - ms_c, ms_e - ms_eb - ms_ec
        part = P.sample_pair_enrichment(7, 0, a.host_samples, annos, anno_off, T, obs)
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, tracks, obs)
        ms_host = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, part)
        ms_d = ms_host * a.samples / a.host_samples
        lines += [
            "%d tracks: %d pairs, %d of them hit by a sample, %d by the input segments (gat_list_pair_hits: %.1f ms); %d intervals in "
            "all; %d batches" % (T, len(obs), int((got[:, 0] > 0).sum()), int((obs > 0).sum()), ms_obs, len(annos), batches),
            "    (a) gat_sample_pair_enrichment end to end           %9.1f ms  (%.1f .. %.1f)" % (ms_a, a0, a1),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, b0, b1),
            "    (c) the same call over one sample (tracks and obs up, words down: %d KB) %9.1f ms  (%.1f .. %.1f)" % (
                got.nbytes >> 10, ms_c, c0, c1),
            "        (a) - (b) - (c): k_pairs over the samples       %9.1f ms = %.2f x the sampler" % (k_pairs, k_pairs / max(ms_b, 1e-9)),
            "    (e) gat_sample_distances, direction 0, end to end   %9.1f ms  (%.1f .. %.1f); its sampler %.1f ms, over one sample %.1f ms" % (
                ms_e, e0, e1, ms_eb, ms_ec),
            "        k_distance over the samples (the searches alone) %8.1f ms; k_pairs / k_distance = %.2f" % (
                k_distance, k_pairs / max(k_distance, 1e-9)),
            "    (d) Problem.sample + numpy, %d samples: %.1f ms (%d segments), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, a.samples, ms_d),
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
