#!/usr/bin/env python
"""Time gat_sample_reldist_enrichment on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one
workspace segment per contig), SamplerAnnotator, against --tracks synthetic point tracks of --points points each (the midpoints
of the intervals tools/time_distance.py searches), at every --bins B:

  (a) the call end to end (wall clock around Problem.sample_reldist_enrichment: the points and obs up, the sampler, k_reldist
      behind every batch, k_null_finish, the five words per (track, value) down),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone (gat_ctx_set_kernel_times),
  (c) the same call over ONE sample -- the fixed cost of a call, so (a) - (b) - (c) is close to what k_reldist costs over the
      samples,
  (d) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists -- a searchsorted per
      (list, track, contig), the bins counted, the area formed, the five words added -- on --host-samples samples, scaled,
  (e) the yardstick: gat_sample_distances (direction 0) in the same session over the same sampled lists against the intervals
      the points come from, (a) - (b) of it as tools/time_distance.py has it: k_distance does the same one search per segment.

Medians over the repeats; the first call warms up.  The words of (a)'s route and (d) over the host route's samples are compared
on the way.

--sweep adds (a) - (b) - (c) under the two context options: what the staging limit and the run of lists are worth.

    python tools/time_reldist.py [--samples 10000] [--host-samples 20] [--tracks 10] [--points 2000] [--reps 3]
                                 [--bins 50 --bins 1024] [--sweep] [--out profiles/r27_reldist.txt]
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
AREA_SCALE = 10 ** 6


def host_counts(a, p, B):
    """(the bins int64 [B], outside) of the SEG array a against the ascending points p (int64) of one contig"""
    a = a[a["end"] > a["start"]]
    if len(a) == 0:
        return np.zeros(B, dtype=np.int64), 0
    s, e = a["start"].astype(np.int64), a["end"].astype(np.int64)
    m = s + (e - s) // 2
    j = np.searchsorted(p, m, side="right")
    inside = (j >= 1) & (j <= len(p) - 1)
    m, j = m[inside], j[inside]
    if len(m) == 0:
        return np.zeros(B, dtype=np.int64), int(len(a))
    lo, hi = p[j - 1], p[j]
    b = np.minimum(B - 1, 2 * np.minimum(m - lo, hi - m) * B // (hi - lo))
    return np.bincount(b, minlength=B), int(len(a) - len(m))


def host_route(P, seed, n_samples, points, B, obs):
    """points[t][c]: int64 positions.  Returns (int64 [n_tracks, B + 3, 5], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    out = np.zeros((len(points), B + 3, 5), dtype=np.int64)
    edges = np.arange(1, B + 1, dtype=np.int64)
    for i in range(n_samples):
        v = np.zeros((len(points), B + 3), dtype=np.int64)
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            for t, per in enumerate(points):
                h, o = host_counts(a, per[c], B)
                v[t, :B] += h
                v[t, B + 2] += o
        n = v[:, :B].sum(axis=1)
        D = np.abs(B * np.cumsum(v[:, :B], axis=1) - edges[None] * n[:, None]).sum(axis=1)
        v[:, B] = [int(d) * AREA_SCALE // (int(k) * B * B) if k else 0 for d, k in zip(D, n)]
        v[:, B + 1] = n
        out[..., 0] += v > 0
        out[..., 1] += v
        out[..., 2] += v * v
        out[..., 3] += v < obs
        out[..., 4] += v == obs
    return out, len(seg)


def median(x):
    x = sorted(x)
    return x[len(x) // 2], x[0], x[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=20)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bins", action="append", type=int)
    ap.add_argument("--sweep", action="store_true", help="k_reldist's time under the context options as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_reldist.txt"))
    a = ap.parse_args()
    all_bins = a.bins or [50, 1024]
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    tracks, points = [], []
    for t in range(a.tracks):
        per = synthetic.random_segments(synthetic.HG19, a.points, 300, 200 + t)
        tracks.append([intervals.normalize(per[c]) if c in per else intervals.EMPTY for c in contigs])
        points.append([x["start"].astype(np.int64) + (x["end"].astype(np.int64) - x["start"].astype(np.int64)) // 2 for x in tracks[-1]])
    lists = [x for per in tracks for x in per]
    annos = np.concatenate(lists)
    anno_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    pos = np.concatenate([p for row in points for p in row]).astype(np.uint32)
    segs = [intervals.normalize(cfg["segments"][c]) if c in cfg["segments"] else intervals.EMPTY for c in contigs]
    seg_all = np.concatenate(segs)
    seg_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_reldist.py --samples %d --host-samples %d --tracks %d --points %d --reps %d %s" % (
                 a.samples, a.host_samples, a.tracks, a.points, a.reps,
                 " ".join(["--bins %d" % b for b in all_bins] + (["--sweep"] if a.sweep else []))),
             "gat_sample_reldist_enrichment on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, %d point "
             "tracks of %d points in all, MI355X, one GPU" % (flat["n_units"], len(flat["segs"]), a.samples, a.tracks, len(pos))]
    # (e) the yardstick, over the same sampled lists
    wall, sampler = [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        P.sample_distances(7, 0, a.samples, annos, anno_off, a.tracks, 0, MAX_DISTANCE)
        wall.append((time.perf_counter() - t0) * 1e3)
        sampler.append(P.last_stats["ms_sampler"])
    ms_dist = median(wall[1:])[0] - median(sampler[1:])[0]
    lines.append("(e) gat_sample_distances, direction 0, the intervals the points come from: end to end %.1f ms, ms_sampler %.1f ms; "
                 "k_distance and the copy of the words %.1f ms" % (median(wall[1:])[0], median(sampler[1:])[0], ms_dist))
    for B in all_bins:
        t0 = time.perf_counter()
        obs = ctx.list_reldist(seg_all, seg_off, 1, pos, anno_off, a.tracks, len(contigs), B)[0]
        ms_obs = (time.perf_counter() - t0) * 1e3
        wall, sampler, fixed = [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_reldist_enrichment(7, 0, a.samples, pos, anno_off, a.tracks, B, obs)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
            batches = P.last_stats["n_batches"]
            t0 = time.perf_counter()
            P.sample_reldist_enrichment(7, 0, 1, pos, anno_off, a.tracks, B, obs)
            fixed.append((time.perf_counter() - t0) * 1e3)
        (ms_a, a_lo, a_hi), (ms_b, b_lo, b_hi), (ms_c, c_lo, c_hi) = median(wall[1:]), median(sampler[1:]), median(fixed[1:])
        part = P.sample_reldist_enrichment(7, 0, a.host_samples, pos, anno_off, a.tracks, B, obs)
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, points, B, obs)
        ms_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        P.sample(7, 0, a.host_samples)
        ms_copy = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, part)
        ms_d = ms_host * a.samples / a.host_samples
        ms_k = ms_a - ms_b - ms_c
        lines += [
            "%d bins: %d values x %d tracks = %d (track, value) cells, %d of them reached by a sample; observed inside %d, outside %d "
            "(gat_list_reldist: %.1f ms); %d batches" % (B, B + 3, a.tracks, (B + 3) * a.tracks, int((got[..., 0] > 0).sum()),
                                                        int(obs[:, B + 1].sum()), int(obs[:, B + 2].sum()), ms_obs, batches),
            "    (a) gat_sample_reldist_enrichment end to end        %9.1f ms  (%.1f .. %.1f)" % (ms_a, a_lo, a_hi),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, b_lo, b_hi),
            "    (c) the same call over one sample (points and obs up, words down) %9.1f ms  (%.1f .. %.1f)" % (ms_c, c_lo, c_hi),
            "        (a) - (b) - (c): k_reldist over the samples     %9.1f ms = %.2f x the sampler = %.2f x (e) k_distance" % (
                ms_k, ms_k / max(ms_b, 1e-9), ms_k / max(ms_dist, 1e-9)),
            "    (d) Problem.sample + numpy, %d samples: %.1f ms (%d segments; the copy-out alone %.1f ms), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, ms_copy, a.samples, ms_d),
            "        (d) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_d / ms_a, a.host_samples,
                                                                                            "equal" if same else "DIFFERENT"),
            "    a list reaches %.1f of the %d bins of a track on average (each a fold of five LDS adds), %.1f segments a bin" % (
                got[:, :B, 0].sum() / (a.samples * a.tracks), B, got[:, :B, 1].sum() / max(1, got[:, :B, 0].sum())),
        ]
        if not a.sweep:
            continue

        def kernel_ms(**options):
            """(a) - (b) - (c) under context options, which change no result"""
            for key, value in options.items():
                ctx.options[key] = value
            try:
                wall, sampler, fixed = [], [], []
                for r in range(a.reps + 1):
                    t0 = time.perf_counter()
                    words = P.sample_reldist_enrichment(7, 0, a.samples, pos, anno_off, a.tracks, B, obs)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    sampler.append(P.last_stats["ms_sampler"])
                    t0 = time.perf_counter()
                    P.sample_reldist_enrichment(7, 0, 1, pos, anno_off, a.tracks, B, obs)
                    fixed.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(words, got)
                return median(wall[1:])[0] - median(sampler[1:])[0] - median(fixed[1:])[0]
            finally:
                for key in options:
                    del ctx.options[key]

        lines.append("    k_reldist over the samples, (a) - (b) - (c), under the context options:")
        for value in ("0", "4", "64"):
            lines.append("        GAT_RELDIST_LDS_POINTS=%-5s             %9.1f ms" % (value, kernel_ms(GAT_RELDIST_LDS_POINTS=value)))
        for value in ("4", "16", "64", "256", "1024"):
            lines.append("        GAT_RELDIST_SAMPLES_PER_BLOCK=%-5s      %9.1f ms" % (value, kernel_ms(GAT_RELDIST_SAMPLES_PER_BLOCK=value)))
    P.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
