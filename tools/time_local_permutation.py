#!/usr/bin/env python
"""Time SamplerLocalPermutation next to SamplerGlobalPermutation on the same inputs: gat_sample_and_count on a synthetic
config shape (default config2: 10 k segments, one workspace piece per contig) or on the reference's test data
(tests/golden/refdata: a workspace of 279 057 pieces), the two samplers alternating in one process, device time of the
whole call (gat_stats::ms_total).  The local sampler is timed in both variants of its kernel -- small pieces resolved in
batches (the default) and one piece per wave step (context option GAT_LPERM_SIMPLE) -- and each of them once more without
the final sort and merge (GAT_EXP_LPERM_NO_NORMALIZE: empty lists, the draw chain alone), which times the two phases apart.
One JSON line per row: the median of the repeats as samples per second, the lowest and highest repeat (the run-to-run
spread), and the words drawn.

    python tools/time_local_permutation.py [--input config2|refdata] [--samples 1000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gat_amd                                   # noqa: E402
from gat_amd import _lib, problem, synthetic     # noqa: E402


def refdata_flat():
    d = os.path.join(ROOT, "tests", "golden", "refdata")
    opts, _ = gat_amd.buildParser().parse_args(["--segments=%s" % os.path.join(d, "segments_single.bed.gz"),
                                                "--annotations=%s" % os.path.join(d, "annotations.bed.gz"),
                                                "--workspace=%s" % os.path.join(d, "workspace.bed.gz"), "--with-segment-tracks"])
    segments, annotations, workspaces, isochores = gat_amd.IO.buildSegments(opts)
    workspace = gat_amd.IO.applyIsochores(segments, annotations, workspaces, opts, isochores)
    track = list(segments.tracks)[0]
    flat = problem.flatten_units(segments[track].asArrays(), workspace.asArrays(),
                                 [(t, annotations[t].asArrays()) for t in annotations.tracks])
    return flat, "nucleotide-overlap"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="config2")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.input == "refdata":
        base, counter = refdata_flat()
    else:
        cfg = synthetic.config(a.input)
        base = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"])
        counter = cfg["counter"]
    ctx = _lib.Context(0)
    knobs = ("GAT_LPERM_SIMPLE", "GAT_EXP_LPERM_NO_NORMALIZE")
    rows = [("global-permutation", 3, ()), ("local-permutation", 4, ()), ("local-permutation simple", 4, knobs[:1]),
            ("local-permutation, draws only", 4, knobs[1:]), ("local-permutation simple, draws only", 4, knobs)]
    probs = {3: _lib.Problem(ctx, dict(base, sampler=3)), 4: _lib.Problem(ctx, dict(base, sampler=4))}
    for P in probs.values():
        P.sample_and_count([counter], 1, 0, min(a.samples, 100))                      # warm-up (tables, scratch)
    times, draws, lines = dict((r[0], []) for r in rows), {}, []
    for r in range(a.reps):
        for label, kind, on in rows:                                                  # alternating, same call shape
            for k in knobs:
                ctx.options.pop(k, None)
            for k in on:
                ctx.options[k] = "1"
            probs[kind].sample_and_count([counter], 100 + r, 0, a.samples)
            times[label].append(probs[kind].last_stats["ms_total"])
            draws[label] = probs[kind].last_stats["n_draws"]
    for k in knobs:
        ctx.options.pop(k, None)
    for label, kind, on in rows:
        v = sorted(times[label])
        lines.append(dict(input=a.input, sampler=label, samples=a.samples, reps=a.reps,
                          samples_per_s=round(a.samples / v[len(v) // 2] * 1e3, 1), ms_median=round(v[len(v) // 2], 3),
                          ms_min=round(v[0], 3), ms_max=round(v[-1], 3), n_draws=draws[label]))
        print(json.dumps(lines[-1]), flush=True)
    for P in probs.values():
        P.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
