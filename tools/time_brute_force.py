#!/usr/bin/env python
"""Time SamplerBruteForce next to SamplerAnnotator on the same problem: gat_sample_and_count on the config-2 geometry with
every segment's length redrawn uniformly from 1..40 (with the config's own lengths -- hundreds of bases -- the brute-force
sampler seldom converges: DESIGN §5 "k_brute_force"), otherwise synthetic.config("config2").  The two samplers alternate in
one process; device time of the whole call (gat_stats::ms_total) and of the sampler's kernels, fromIsochores and the count
kernels (gat_ctx_set_kernel_times), medians over the repeats.  A call in which some work unit does not converge fails as
the reference's run would: it is reported (n_unconverged) and the repeat takes the next seed.

    python tools/time_brute_force.py [--samples 1000] [--reps 5] [--out profiles/r10_brute_force.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gat_amd import _lib, problem, synthetic     # noqa: E402


def short_segments(segments, seed=1, maxlen=40):
    r = np.random.RandomState(seed)
    out = type(segments)()
    for c, a in segments.items():
        a = a.copy()
        nxt = np.append(a["start"][1:], np.iinfo(np.int64).max)
        a["end"] = np.minimum(a["start"].astype(np.int64) + r.randint(1, maxlen + 1, len(a)), nxt).astype(a["end"].dtype)
        out[c] = a
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    cfg = synthetic.config("config2")
    base = problem.flatten_arrays(short_segments(cfg["segments"]), cfg["annotations"], cfg["workspace"], cfg["isochores"],
                                  bucket_size=1)
    counters = [cfg["counter"]]
    keys = ("ms_total", "ms_sampler", "ms_contig", "ms_count")
    probs, times, failed = {}, {}, {}
    for kind, label in ((0, "annotator"), (5, "brute-force")):
        probs[label] = _lib.Problem(ctx, dict(base, sampler=kind))
        times[label], failed[label] = [], 0
    seed = 100
    for r in range(a.reps + 1):                                                      # (the first round warms up)
        for label, P in probs.items():
            for _ in range(20):
                seed += 1
                try:
                    P.sample_and_count(counters, seed, 0, a.samples)
                    break
                except ValueError:
                    failed[label] += P.last_stats["n_unconverged"]
            else:
                raise SystemExit("%s: 20 seeds in a row did not converge" % label)
            if r:
                times[label].append(dict(P.last_stats))
    lines = []
    for label, P in probs.items():
        med = dict((k, sorted(t[k] for t in times[label])[len(times[label]) // 2]) for k in keys)
        st = times[label][-1]
        lines.append(dict(shape="config2, segment lengths 1..40", sampler=label, samples=a.samples, reps=a.reps,
                          units=P.n_units, ms=dict((k, round(v, 3)) for k, v in med.items()),
                          samples_per_s=round(a.samples / med["ms_total"] * 1000.0), n_placed=st["n_placed"], n_draws=st["n_draws"],
                          n_rejected_tries=st["n_unsuccessful"] if label == "brute-force" else None, n_restarts=st["n_restarts"],
                          n_retried=st["n_retried"], unconverged_units_in_failed_calls=failed[label]))
        P.close()
    lines.append(dict(brute_force_over_annotator=round(lines[1]["ms"]["ms_total"] / lines[0]["ms"]["ms_total"], 2)))
    ctx.close()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
