#!/usr/bin/env python
"""Time gat_sample_profile_enrichment on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one
workspace segment per contig), SamplerAnnotator, around --tracks synthetic anchor tracks of --anchors stranded anchors each (the
five-prime ends of the intervals tools/time_distance.py searches, strands alternating), at every --geometry bin_size,half_bins:

  (a) the call end to end (wall clock around Problem.sample_profile_enrichment: the anchors and obs up, the sampler, k_profile
      behind every batch, k_null_finish, the five words per (track, bin) down),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone (gat_ctx_set_kernel_times),
  (c) the same call over ONE sample -- the fixed cost of a call, so (a) - (b) - (c) is close to what k_profile costs over the
      samples,
  (d) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists -- every (segment,
      anchor) pair within reach clipped to the window, cut at the bin edges and added into the five words -- on --host-samples
      samples, scaled,
  (e) the yardstick: gat_sample_distances (direction 0) in the same session over the same sampled lists against the intervals
      the anchors come from, (a) - (b) of it as tools/time_distance.py has it: k_distance does the same one search per segment
      without the window adds.

Medians over the repeats; the first call warms up.  The words of (a)'s route and (d) over the host route's samples are compared
on the way.

--sweep adds (a) - (b) - (c) under the two context options and for GAT_PROFILE_MIDPOINTS: what the staging limit, the run of
lists and the window adds are worth.

    python tools/time_profile.py [--samples 10000] [--host-samples 20] [--tracks 10] [--anchors 2000] [--reps 3]
                                 [--geometry 100,50 --geometry 10,512] [--sweep] [--out profiles/r22_profile.txt]
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


def host_values(a, pos, minus, w, H):
    """v[2 H] of the normalized SEG array a around the anchors (pos ascending, minus 0 / 1) of one contig"""
    B, R = 2 * H, H * w
    out = np.zeros(B, dtype=np.int64)
    if len(a) == 0 or len(pos) == 0:
        return out
    s, e = a["start"].astype(np.int64), a["end"].astype(np.int64)
    p = pos.astype(np.int64)
    lo, hi = np.searchsorted(p, s - R, side="left"), np.searchsorted(p, e + R, side="left")
    n = hi - lo
    if n.sum() == 0:
        return out
    first = np.repeat(np.cumsum(n) - n, n)
    k = np.repeat(lo, n) + (np.arange(int(n.sum())) - first)             # the anchor of every (segment, anchor) pair
    s, e, anchor, m = np.repeat(s, n), np.repeat(e, n), p[k], minus[k].astype(bool)
    wlo = np.where(m, anchor - R + 1, anchor - R)                        # the window's bases [wlo, wlo + 2 R)
    cs, ce = np.maximum(s, wlo), np.minimum(e, wlo + 2 * R)
    keep = ce > cs
    cs, ce, wlo, m = cs[keep], ce[keep], wlo[keep], m[keep]
    us, ue = np.where(m, wlo + 2 * R - ce, cs - wlo), np.where(m, wlo + 2 * R - cs, ce - wlo)
    fb, lb = us // w, (ue - 1) // w
    reps = lb - fb + 1
    first = np.repeat(np.cumsum(reps) - reps, reps)
    b = np.repeat(fb, reps) + (np.arange(int(reps.sum())) - first)
    ps, pe = np.maximum(np.repeat(us, reps), b * w), np.minimum(np.repeat(ue, reps), (b + 1) * w)
    return np.bincount(b, weights=(pe - ps).astype(np.float64), minlength=B).astype(np.int64)


def host_route(P, seed, n_samples, anchors, w, H, obs):
    """anchors[t][c]: (pos, minus).  Returns (int64 [n_tracks, 2 H, 5], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C = P.n_contigs
    out = np.zeros((len(anchors), 2 * H, 5), dtype=np.int64)
    for i in range(n_samples):
        v = np.zeros((len(anchors), 2 * H), dtype=np.int64)
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            for t, per in enumerate(anchors):
                v[t] += host_values(a, per[c][0], per[c][1], w, H)
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
    ap.add_argument("--anchors", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--geometry", action="append", help="bin_size,half_bins")
    ap.add_argument("--sweep", action="store_true", help="k_profile's time under the context options as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_profile.txt"))
    a = ap.parse_args()
    geometries = [tuple(int(x) for x in g.split(",")) for g in (a.geometry or ["100,50", "10,512"])]
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    tracks, anchors = [], []
    for t in range(a.tracks):
        per = synthetic.random_segments(synthetic.HG19, a.anchors, 300, 200 + t)
        tracks.append([intervals.normalize(per[c]) if c in per else intervals.EMPTY for c in contigs])
        row = []
        for x in tracks[-1]:                           # five-prime ends, strands alternating along the contig
            minus = (np.arange(len(x)) % 2).astype(np.uint8)
            pos = np.where(minus == 1, x["end"].astype(np.int64) - 1, x["start"].astype(np.int64))
            order = np.argsort(pos * 2 + minus, kind="stable")
            row.append((pos[order].astype(np.uint32), minus[order]))
        anchors.append(row)
    lists = [x for per in tracks for x in per]
    annos = np.concatenate(lists)
    anno_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    pos = np.concatenate([p for row in anchors for p, _ in row])
    minus = np.concatenate([m for row in anchors for _, m in row])
    segs = [intervals.normalize(cfg["segments"][c]) if c in cfg["segments"] else intervals.EMPTY for c in contigs]
    seg_all = np.concatenate(segs)
    seg_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_profile.py --samples %d --host-samples %d --tracks %d --anchors %d --reps %d %s" % (
                 a.samples, a.host_samples, a.tracks, a.anchors, a.reps,
                 " ".join(["--geometry %d,%d" % g for g in geometries] + (["--sweep"] if a.sweep else []))),
             "gat_sample_profile_enrichment on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, %d anchor "
             "tracks of %d stranded anchors in all, MI355X, one GPU" % (flat["n_units"], len(flat["segs"]), a.samples, a.tracks, len(pos))]
    # (e) the yardstick, over the same sampled lists
    wall, sampler = [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        P.sample_distances(7, 0, a.samples, annos, anno_off, a.tracks, 0, MAX_DISTANCE)
        wall.append((time.perf_counter() - t0) * 1e3)
        sampler.append(P.last_stats["ms_sampler"])
    ms_dist = median(wall[1:])[0] - median(sampler[1:])[0]
    lines.append("(e) gat_sample_distances, direction 0, the intervals the anchors come from: end to end %.1f ms, ms_sampler %.1f ms; "
                 "k_distance and the copy of the words %.1f ms" % (median(wall[1:])[0], median(sampler[1:])[0], ms_dist))
    for w, H in geometries:
        t0 = time.perf_counter()
        obs = ctx.list_profile(seg_all, seg_off, 1, pos, minus, anno_off, a.tracks, len(contigs), w, H, 0)[0]
        ms_obs = (time.perf_counter() - t0) * 1e3
        wall, sampler, fixed = [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_profile_enrichment(7, 0, a.samples, pos, minus, anno_off, a.tracks, w, H, 0, obs)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
            batches = P.last_stats["n_batches"]
            t0 = time.perf_counter()
            P.sample_profile_enrichment(7, 0, 1, pos, minus, anno_off, a.tracks, w, H, 0, obs)
            fixed.append((time.perf_counter() - t0) * 1e3)
        (ms_a, a_lo, a_hi), (ms_b, b_lo, b_hi), (ms_c, c_lo, c_hi) = median(wall[1:]), median(sampler[1:]), median(fixed[1:])
        part = P.sample_profile_enrichment(7, 0, a.host_samples, pos, minus, anno_off, a.tracks, w, H, 0, obs)
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, anchors, w, H, obs)
        ms_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        P.sample(7, 0, a.host_samples)
        ms_copy = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, part)
        ms_d = ms_host * a.samples / a.host_samples
        ms_k = ms_a - ms_b - ms_c
        lines += [
            "bin_size %d, half_bins %d: %d bins x %d tracks = %d (track, bin) cells, %d of them reached by a sample, %d with an "
            "observed base (gat_list_profile: %.1f ms); %d batches" % (w, H, 2 * H, a.tracks, 2 * H * a.tracks, int((got[..., 0] > 0).sum()),
                                                                       int((obs > 0).sum()), ms_obs, batches),
            "    (a) gat_sample_profile_enrichment end to end        %9.1f ms  (%.1f .. %.1f)" % (ms_a, a_lo, a_hi),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, b_lo, b_hi),
            "    (c) the same call over one sample (anchors and obs up, words down) %9.1f ms  (%.1f .. %.1f)" % (ms_c, c_lo, c_hi),
            "        (a) - (b) - (c): k_profile over the samples     %9.1f ms = %.2f x the sampler = %.2f x (e) k_distance" % (
                ms_k, ms_k / max(ms_b, 1e-9), ms_k / max(ms_dist, 1e-9)),
            "    (d) Problem.sample + numpy, %d samples: %.1f ms (%d segments; the copy-out alone %.1f ms), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, ms_copy, a.samples, ms_d),
            "        (d) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_d / ms_a, a.host_samples,
                                                                                            "equal" if same else "DIFFERENT"),
            "    a list reaches %.1f of the %d bins of a track on average (each a fold of five LDS adds), %.1f bases a bin" % (
                got[..., 0].sum() / (a.samples * a.tracks), 2 * H, got[..., 1].sum() / max(1, got[..., 0].sum())),
        ]
        if not a.sweep:
            continue

        def kernel_ms(mode=0, **options):
            """(a) - (b) - (c) under context options, which change no result"""
            for key, value in options.items():
                ctx.options[key] = value
            try:
                wall, sampler, fixed = [], [], []
                for r in range(a.reps + 1):
                    t0 = time.perf_counter()
                    words = P.sample_profile_enrichment(7, 0, a.samples, pos, minus, anno_off, a.tracks, w, H, mode, obs)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    sampler.append(P.last_stats["ms_sampler"])
                    t0 = time.perf_counter()
                    P.sample_profile_enrichment(7, 0, 1, pos, minus, anno_off, a.tracks, w, H, mode, obs)
                    fixed.append((time.perf_counter() - t0) * 1e3)
                assert mode != 0 or np.array_equal(words, got)
                return median(wall[1:])[0] - median(sampler[1:])[0] - median(fixed[1:])[0]
            finally:
                for key in options:
                    del ctx.options[key]

        lines.append("    k_profile over the samples, (a) - (b) - (c), under the context options:")
        for value in ("0", "4", "64"):
            lines.append("        GAT_PROFILE_LDS_ANCHORS=%-5s            %9.1f ms" % (value, kernel_ms(GAT_PROFILE_LDS_ANCHORS=value)))
        for value in ("4", "16", "64", "256", "1024"):
            lines.append("        GAT_PROFILE_SAMPLES_PER_BLOCK=%-5s      %9.1f ms" % (value, kernel_ms(GAT_PROFILE_SAMPLES_PER_BLOCK=value)))
        lines.append("        GAT_PROFILE_MIDPOINTS (one base a segment: the searches and the walk, next to no window adds) %9.1f ms" % kernel_ms(1))
    P.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
