#!/usr/bin/env python
"""Time SamplerUniverse beside SamplerAnnotator and SamplerCircular on the same problems: gat_sample_and_count, the three
samplers alternating in one process, device time of the whole call (gat_stats::ms_total, events on the library's stream).

  peaks     a universe of 100 000 candidate regions of about 500 bases on the config-2 contigs (hg19), 10 000 of them the
            segments, config 2's annotation track
  refdata   the reference's test data: the fragmented workspace as the universe, the 8 549-segment track as the segments

One JSON line per (shape, sampler): the median of the repeats per 10 000 samples, and the sampler stage alone (ms_sampler) of
one further call with the per-kernel events on; then the ratios and the shape (units, pieces, hit pieces).

    python tools/time_universe.py [--samples 10000] [--reps 3] [--configs peaks,refdata] [--out profiles/r28_universe.txt]
"""
import argparse
import collections
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gat_amd import _lib, problem, synthetic     # noqa: E402

SAMPLERS = ((0, "annotator"), (6, "circular"), (7, "universe"))


def peaks(n_universe=100000, n_segments=10000, seed=28):
    """the universe, and a uniform subset of it as the segments"""
    universe = synthetic.random_segments(synthetic.HG19, n_universe, 500, seed)
    rs = np.random.RandomState(seed + 1)
    total = sum(len(a) for a in universe.values())
    pick = np.zeros(total, dtype=bool)
    pick[rs.choice(total, size=min(n_segments, total), replace=False)] = True
    segments, at = collections.OrderedDict(), 0
    for contig, a in universe.items():
        mine = a[pick[at:at + len(a)]]
        at += len(a)
        if len(mine):
            segments[contig] = mine
    return dict(segments=segments, annotations=[("anno0", synthetic.random_segments(synthetic.HG19, 10000, 2000, 100))],
                workspace=universe, isochores=None, counter="nucleotide-overlap")


def hit_pieces(flat):
    """k over the units: the pieces that share a base with a segment"""
    k = 0
    for u in range(int(flat["n_units"])):
        s = flat["segs"][flat["seg_off"][u]:flat["seg_off"][u + 1]]
        w = flat["ws"][flat["ws_off"][u]:flat["ws_off"][u + 1]]
        if len(s) == 0 or len(w) == 0:
            continue
        first = np.searchsorted(s["end"], w["start"], side="right")            # the first segment ending beyond the piece's start
        k += int(np.count_nonzero((first < len(s)) & (s["start"][np.minimum(first, len(s) - 1)] < w["end"])))
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="peaks,refdata")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    lines = []
    for name in a.configs.split(","):
        cfg = peaks() if name == "peaks" else synthetic.config(name)
        base = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"])
        counters = [cfg["counter"]]
        probs = {}
        for kind, label in SAMPLERS:
            probs[label] = _lib.Problem(ctx, dict(base, sampler=kind))
            probs[label].sample_and_count(counters, 1, 0, min(a.samples, 1000))       # warm-up (tables, scratch)
        total = dict((k, []) for k in probs)
        for r in range(a.reps):
            for label, P in probs.items():                                            # alternating, same call shape
                P.sample_and_count(counters, 100 + r, 0, a.samples)
                total[label].append(P.last_stats["ms_total"] * 10000.0 / a.samples)
        med = dict((k, sorted(v)[len(v) // 2]) for k, v in total.items())
        ctx.set_kernel_times(True)                                                    # (an event behind every kernel: not in the medians)
        stage = {}
        for label, P in probs.items():
            P.sample_and_count(counters, 99, 0, a.samples)
            stage[label] = P.last_stats["ms_sampler"] * 10000.0 / a.samples
        ctx.set_kernel_times(False)
        first = len(lines)
        for label, P in probs.items():
            st = P.last_stats
            lines.append(dict(config=name, sampler=label, samples=a.samples, reps=a.reps, ms_total_per_10k=round(med[label], 3),
                              ms_sampler_per_10k=round(stage[label], 3), n_draws=st["n_draws"], n_retried=st["n_retried"]))
            P.close()
        lines.append(dict(config=name, units=int(base["n_units"]), pieces=int(len(base["ws"])), segments=int(len(base["segs"])),
                          hit_pieces=hit_pieces(base), universe_over_annotator=round(med["universe"] / med["annotator"], 3),
                          universe_over_circular=round(med["universe"] / med["circular"], 3)))
        for l in lines[first:]:
            print(json.dumps(l), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
