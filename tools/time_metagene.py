#!/usr/bin/env python
"""Time gat_sample_metagene_enrichment on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one
workspace segment per contig), SamplerAnnotator, along --tracks synthetic feature tracks of --features stranded features each
(the intervals tools/time_distance.py searches, strands alternating), at every --geometry body_bins,flank_bins,flank_bin_size:

  (a) the call end to end (wall clock around Problem.sample_metagene_enrichment: the features and obs up, the sampler,
      k_metagene behind every batch, k_null_finish, the five words per (track, bin) down),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone (gat_ctx_set_kernel_times),
  (c) the same call over ONE sample -- the fixed cost of a call, so (a) - (b) - (c) is close to what k_metagene costs over the
      samples,
  (d) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists -- every (segment,
      feature) pair within reach clipped to the window, cut at the bin edges and added into the five words -- on --host-samples
      samples, scaled,
  (e) the yardsticks, in the same session over the same sampled lists: gat_sample_profile_enrichment around the features'
      five-prime ends at --profile-geometry bin_size,half_bins ((a) - (b) - (c) of it, as tools/time_profile.py has it), and
      gat_sample_distances (direction 0) against the same intervals ((a) - (b) of it, as tools/time_distance.py has it),
  (f) --nested: the same call with one more feature per (track, contig) that spans the first half of the contig (the whole
      contig would pass the sumsq bound at 10 000 samples), under which the features of that half are nested: the prefix
      maximum of the ends is the middle of the contig from the first feature on, the search finds feature 0 for every segment
      of that half and the walk passes over every feature that starts before the segment.

Medians over the repeats; the first call warms up.  The words of (a)'s route and (d) over the host route's samples are compared
on the way.

--sweep adds (a) - (b) - (c) under the two context options and for GAT_METAGENE_MIDPOINTS.

    python tools/time_metagene.py [--samples 10000] [--host-samples 5] [--tracks 10] [--features 2000] [--reps 3]
                                  [--geometry 50,20,100 --geometry 1024,0,1] [--nested] [--sweep] [--out profiles/r29_metagene.txt]
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


def host_values(a, fs, fe, minus, Bb, Bf, w):
    """v[B] of the normalized SEG array a along the features (ascending by start, minus 0 / 1) of one contig"""
    B, F = 2 * Bf + Bb, Bf * w
    out = np.zeros(B, dtype=np.int64)
    if len(a) == 0 or len(fs) == 0:
        return out
    s, e = a["start"].astype(np.int64), a["end"].astype(np.int64)
    fs, fe = fs.astype(np.int64), fe.astype(np.int64)
    lo, hi = np.searchsorted(np.maximum.accumulate(fe), s - F, side="right"), np.searchsorted(fs, e + F, side="left")
    n = np.maximum(hi - lo, 0)
    if n.sum() == 0:
        return out
    first = np.repeat(np.cumsum(n) - n, n)
    k = np.repeat(lo, n) + (np.arange(int(n.sum())) - first)             # the feature of every (segment, feature) pair
    s, e, a0, a1, m = np.repeat(s, n), np.repeat(e, n), fs[k], fe[k], minus[k].astype(bool)
    cs, ce = np.maximum(s, a0 - F), np.minimum(e, a1 + F)
    keep = ce > cs
    cs, ce, a0, a1, m = cs[keep], ce[keep], a0[keep], a1[keep], m[keep]
    length = a1 - a0
    us, ue = np.where(m, a1 + F - ce, cs - (a0 - F)), np.where(m, a1 + F - cs, ce - (a0 - F))

    def bin_of(u, length):
        return np.where(u < F, u // w, np.where(u < F + length, Bf + (u - F) * Bb // length, Bf + Bb + (u - F - length) // w))

    def start_of(b, length):                                            # the oriented offset at which bin b begins
        return np.where(b < Bf, b * w, np.where(b <= Bf + Bb, F - (-((b - Bf) * length) // Bb), F + length + (b - Bf - Bb) * w))

    fb, lb = bin_of(us, length), bin_of(ue - 1, length)
    reps = lb - fb + 1
    first = np.repeat(np.cumsum(reps) - reps, reps)
    b = np.repeat(fb, reps) + (np.arange(int(reps.sum())) - first)
    length = np.repeat(length, reps)
    ps, pe = np.maximum(np.repeat(us, reps), start_of(b, length)), np.minimum(np.repeat(ue, reps), start_of(b + 1, length))
    return np.bincount(b, weights=np.maximum(pe - ps, 0).astype(np.float64), minlength=B).astype(np.int64)


def host_route(P, seed, n_samples, features, Bb, Bf, w, obs):
    """features[t][c]: (fs, fe, minus).  Returns (int64 [n_tracks, B, 5], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C, B = P.n_contigs, 2 * Bf + Bb
    out = np.zeros((len(features), B, 5), dtype=np.int64)
    for i in range(n_samples):
        v = np.zeros((len(features), B), dtype=np.int64)
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            for t, per in enumerate(features):
                v[t] += host_values(a, per[c][0], per[c][1], per[c][2], Bb, Bf, w)
        out[..., 0] += v > 0
        out[..., 1] += v
        out[..., 2] += v * v
        out[..., 3] += v < obs
        out[..., 4] += v == obs
    return out, len(seg)


def median(x):
    x = sorted(x)
    return x[len(x) // 2], x[0], x[-1]


def flat_features(features):
    fs = np.concatenate([x[0] for row in features for x in row])
    fe = np.concatenate([x[1] for row in features for x in row])
    minus = np.concatenate([x[2] for row in features for x in row])
    off = np.concatenate([[0], np.cumsum([len(x[0]) for row in features for x in row])]).astype(np.int64)
    return fs, fe, minus, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=5)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--geometry", action="append", help="body_bins,flank_bins,flank_bin_size")
    ap.add_argument("--profile-geometry", action="append", help="bin_size,half_bins of the k_profile yardstick")
    ap.add_argument("--nested", action="store_true", help="also with one feature over the first half of every contig, the others there nested under it")
    ap.add_argument("--sweep", action="store_true", help="k_metagene's time under the context options as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_metagene.txt"))
    a = ap.parse_args()
    geometries = [tuple(int(x) for x in g.split(",")) for g in (a.geometry or ["50,20,100", "1024,0,1"])]
    profile_geometries = [tuple(int(x) for x in g.split(",")) for g in (a.profile_geometry or ["100,50", "10,512"])]
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    ext = [0] * len(contigs)                                 # per contig: the largest workspace end of its units
    for u, c in enumerate(flat["unit_contig"]):
        ws = flat["ws"][flat["ws_off"][u]:flat["ws_off"][u + 1]]
        if c >= 0 and len(ws):
            ext[c] = max(ext[c], int(ws["end"].max()))
    tracks, features, nested, anchors = [], [], [], []
    for t in range(a.tracks):
        per = synthetic.random_segments(synthetic.HG19, a.features, 300, 200 + t)
        tracks.append([intervals.normalize(per[c]) if c in per else intervals.EMPTY for c in contigs])
        row, row_nested, row_anchors = [], [], []
        for c, x in enumerate(tracks[-1]):                   # the intervals as they are (sorted, disjoint), strands alternating
            fs, fe, minus = x["start"].astype(np.uint32), x["end"].astype(np.uint32), (np.arange(len(x)) % 2).astype(np.uint8)
            row.append((fs, fe, minus))
            key = sorted(zip([0] + fs.tolist(), [max(ext[c] // 2, 1)] + fe.tolist(), [0] + minus.tolist()))
            row_nested.append(tuple(np.array(col, dtype=dt) for col, dt in zip(zip(*key), (np.uint32, np.uint32, np.uint8))))
            pos = np.where(minus == 1, fe.astype(np.int64) - 1, fs.astype(np.int64))
            order = np.argsort(pos * 2 + minus, kind="stable")
            row_anchors.append((pos[order].astype(np.uint32), minus[order]))
        features.append(row)
        nested.append(row_nested)
        anchors.append(row_anchors)
    lists = [x for per in tracks for x in per]
    annos = np.concatenate(lists)
    anno_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    fs, fe, minus, feat_off = flat_features(features)
    pos = np.concatenate([p for row in anchors for p, _ in row])
    pos_minus = np.concatenate([m for row in anchors for _, m in row])
    segs = [intervals.normalize(cfg["segments"][c]) if c in cfg["segments"] else intervals.EMPTY for c in contigs]
    seg_all = np.concatenate(segs)
    seg_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_metagene.py --samples %d --host-samples %d --tracks %d --features %d --reps %d %s" % (
                 a.samples, a.host_samples, a.tracks, a.features, a.reps,
                 " ".join(["--geometry %d,%d,%d" % g for g in geometries] + ["--profile-geometry %d,%d" % g for g in profile_geometries] +
                          (["--nested"] if a.nested else []) + (["--sweep"] if a.sweep else []))),
             "gat_sample_metagene_enrichment on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, %d feature "
             "tracks of %d stranded features in all (mean length %.0f bases, the longest (track, contig) %d), MI355X, one GPU" % (
                 flat["n_units"], len(flat["segs"]), a.samples, a.tracks, len(fs), float((fe.astype(np.int64) - fs).mean()),
                 int(np.diff(feat_off).max()))]

    def timed(call):
        """medians of (end to end, ms_sampler, the same call over one sample), the words, the batches"""
        wall, sampler, fixed = [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            words = call(a.samples)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
            batches = P.last_stats["n_batches"]
            t0 = time.perf_counter()
            call(1)
            fixed.append((time.perf_counter() - t0) * 1e3)
        return median(wall[1:]), median(sampler[1:]), median(fixed[1:]), words, batches

    # (e) the yardsticks, over the same sampled lists
    wall, sampler = [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        P.sample_distances(7, 0, a.samples, annos, anno_off, a.tracks, 0, MAX_DISTANCE)
        wall.append((time.perf_counter() - t0) * 1e3)
        sampler.append(P.last_stats["ms_sampler"])
    ms_dist = median(wall[1:])[0] - median(sampler[1:])[0]
    lines.append("(e) gat_sample_distances, direction 0, the same intervals: end to end %.1f ms, ms_sampler %.1f ms; "
                 "k_distance and the copy of the words %.1f ms" % (median(wall[1:])[0], median(sampler[1:])[0], ms_dist))
    ms_profile = []
    for w, H in profile_geometries:
        obs = ctx.list_profile(seg_all, seg_off, 1, pos, pos_minus, anno_off, a.tracks, len(contigs), w, H, 0)[0]
        (ms_a, _, _), (ms_b, _, _), (ms_c, _, _), _, _ = timed(
            lambda n: P.sample_profile_enrichment(7, 0, n, pos, pos_minus, anno_off, a.tracks, w, H, 0, obs))
        ms_profile.append(ms_a - ms_b - ms_c)
        lines.append("(e) gat_sample_profile_enrichment around the features' five-prime ends, bin_size %d, half_bins %d (%d bins): end to end "
                     "%.1f ms, ms_sampler %.1f ms, one sample %.1f ms; k_profile over the samples %.1f ms" % (
                         w, H, 2 * H, ms_a, ms_b, ms_c, ms_profile[-1]))
    for g, (Bb, Bf, w) in enumerate(geometries):
        B = 2 * Bf + Bb
        ms_prof = ms_profile[min(g, len(ms_profile) - 1)]
        pw, pH = profile_geometries[min(g, len(profile_geometries) - 1)]
        t0 = time.perf_counter()
        obs = ctx.list_metagene(seg_all, seg_off, 1, fs, fe, minus, feat_off, a.tracks, len(contigs), Bb, Bf, w, 0)[0]
        ms_obs = (time.perf_counter() - t0) * 1e3
        (ms_a, a_lo, a_hi), (ms_b, b_lo, b_hi), (ms_c, c_lo, c_hi), got, batches = timed(
            lambda n: P.sample_metagene_enrichment(7, 0, n, fs, fe, minus, feat_off, a.tracks, Bb, Bf, w, 0, obs))
        part = P.sample_metagene_enrichment(7, 0, a.host_samples, fs, fe, minus, feat_off, a.tracks, Bb, Bf, w, 0, obs)
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, features, Bb, Bf, w, obs)
        ms_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        P.sample(7, 0, a.host_samples)
        ms_copy = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, part)
        ms_d = ms_host * a.samples / a.host_samples
        ms_k = ms_a - ms_b - ms_c
        lines += [
            "body_bins %d, flank_bins %d, flank_bin_size %d: %d bins x %d tracks = %d (track, bin) cells, %d of them reached by a sample, %d "
            "with an observed base (gat_list_metagene: %.1f ms); %d batches" % (Bb, Bf, w, B, a.tracks, B * a.tracks, int((got[..., 0] > 0).sum()),
                                                                              int((obs > 0).sum()), ms_obs, batches),
            "    (a) gat_sample_metagene_enrichment end to end       %9.1f ms  (%.1f .. %.1f)" % (ms_a, a_lo, a_hi),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, b_lo, b_hi),
            "    (c) the same call over one sample (features and obs up, words down) %9.1f ms  (%.1f .. %.1f)" % (ms_c, c_lo, c_hi),
            "        (a) - (b) - (c): k_metagene over the samples    %9.1f ms = %.2f x the sampler = %.2f x (e) k_profile at %d,%d = %.2f x "
            "(e) k_distance" % (ms_k, ms_k / max(ms_b, 1e-9), ms_k / max(ms_prof, 1e-9), pw, pH, ms_k / max(ms_dist, 1e-9)),
            "    (d) Problem.sample + numpy, %d samples: %.1f ms (%d segments; the copy-out alone %.1f ms), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, ms_copy, a.samples, ms_d),
            "        (d) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_d / ms_a, a.host_samples,
                                                                                            "equal" if same else "DIFFERENT"),
            "    a list reaches %.1f of the %d bins of a track on average (each a fold of five LDS adds), %.1f bases a bin" % (
                got[..., 0].sum() / (a.samples * a.tracks), B, got[..., 1].sum() / max(1, got[..., 0].sum())),
        ]
        if a.nested:
            nfs, nfe, nminus, noff = flat_features(nested)
            nobs = ctx.list_metagene(seg_all, seg_off, 1, nfs, nfe, nminus, noff, a.tracks, len(contigs), Bb, Bf, w, 0)[0]
            (n_a, _, _), (n_b, _, _), (n_c, _, _), _, _ = timed(
                lambda n: P.sample_metagene_enrichment(7, 0, n, nfs, nfe, nminus, noff, a.tracks, Bb, Bf, w, 0, nobs))
            lines.append("    (f) with one feature over the first half of every contig and the others there nested under it (%d features; a segment "
                         "of that half walks from feature 0): k_metagene over the samples %9.1f ms = %.2f x (a) - (b) - (c) without it" % (
                             len(nfs), n_a - n_b - n_c, (n_a - n_b - n_c) / max(ms_k, 1e-9)))
        if not a.sweep:
            continue

        def kernel_ms(mode=0, **options):
            """(a) - (b) - (c) under context options, which change no result"""
            for key, value in options.items():
                ctx.options[key] = value
            try:
                (k_a, _, _), (k_b, _, _), (k_c, _, _), words, _ = timed(
                    lambda n: P.sample_metagene_enrichment(7, 0, n, fs, fe, minus, feat_off, a.tracks, Bb, Bf, w, mode, obs))
                assert mode != 0 or np.array_equal(words, got)
                return k_a - k_b - k_c
            finally:
                for key in options:
                    del ctx.options[key]

        lines.append("    k_metagene over the samples, (a) - (b) - (c), under the context options:")
        for value in ("0", "4", "64"):
            lines.append("        GAT_METAGENE_LDS_FEATURES=%-5s          %9.1f ms" % (value, kernel_ms(GAT_METAGENE_LDS_FEATURES=value)))
        for value in ("4", "16", "64", "256"):
            lines.append("        GAT_METAGENE_SAMPLES_PER_BLOCK=%-5s     %9.1f ms" % (value, kernel_ms(GAT_METAGENE_SAMPLES_PER_BLOCK=value)))
        lines.append("        GAT_METAGENE_MIDPOINTS (one base a segment: the searches and the walk, one add) %9.1f ms" % kernel_ms(1))
    P.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
