#!/usr/bin/env python
"""Time SamplerCircular beside SamplerGlobalPermutation and SamplerAnnotator on the same shapes: gat_sample_and_count on the
config-2 and refdata geometries, the three samplers alternating in one process, device time of the whole call
(gat_stats::ms_total, events on the library's stream).  One JSON line per (shape, sampler): the median of the repeats per
10 000 samples, and the sampler stage alone (ms_sampler) of one further call with the per-kernel events on; then the ratios.

    python tools/time_circular.py [--samples 10000] [--reps 3] [--configs config2,refdata] [--out profiles/r26_circular.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gat_amd import _lib, problem, synthetic     # noqa: E402

SAMPLERS = ((0, "annotator"), (3, "global-permutation"), (6, "circular"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="config2,refdata")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    lines = []
    for name in a.configs.split(","):
        cfg = synthetic.config(name)
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
        lines.append(dict(config=name, circular_over_permutation=round(med["circular"] / med["global-permutation"], 3),
                          circular_over_annotator=round(med["circular"] / med["annotator"], 3)))
        for l in lines[first:]:
            print(json.dumps(l), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
