#!/usr/bin/env python
"""Golden vectors at both ends of the coordinate range, taken from the REFERENCE ITSELF -- tests/golden/coordinate_range.json.

Run in the build container only, like make_goldens_brute_force.py:

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_goldens_coordinate_range.py 2> /dev/null

The cases are tests/range_cases.py's (this script holds none of its own and none of the reference's code: it imports both).

  in_domain     per (case, sampler) the inputs and, under "streams", per seed [seed, list, next]: numpy.random.seed(seed), then Sampler*(bucket_size, nbuckets).sample(segments,
                workspace) -- the list as the sampler returned it (flat: start, end, start, end, ...), and the next raw
                32-bit output of the generator (what the sample consumed).  Streams 0 .. 19 of top_tiny (bucket sizes 1
                and 3), bottom, wide_span and frag_top under SamplerAnnotator and SamplerSegments, of top_tiny (bucket 1)
                and bottom_brute under SamplerBruteForce; streams 0 .. 199 of top_tiny (bucket 1) under SamplerAnnotator,
                the ones the placement domain was measured on.
  past_border   EVIDENCE ONLY -- no test expects the library to reproduce any of it (it refuses these inputs): workspaces one
                base and more past the border, the streams run, and for each stream on which the reference raised: the
                seed, the exception's class, the line of gat/Engine.pyx it came from and its text.
"""
import json
import os
import sys
import traceback

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                        # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository (oracle/)

import gat.Engine as Engine                  # noqa: E402  (the reference, from PYTHONPATH)
from gat.SegmentList import SegmentList      # noqa: E402

import range_cases as R                      # noqa: E402

OUT = os.path.join(HERE, "coordinate_range.json")


def make_sampler(kind, bucket_size):
    if kind == R.ANNOTATOR:
        return Engine.SamplerAnnotator(bucket_size=bucket_size, nbuckets=R.NBUCKETS)
    if kind == R.SEGMENTS:
        return Engine.SamplerSegments(bucket_size=bucket_size, nbuckets=R.NBUCKETS)
    return Engine.SamplerBruteForce(bucket_size, R.NBUCKETS, 100, 10)


def reference(kind, bucket_size, segs, ws, seed):
    """(flat list, next raw output), or the exception where the reference raises."""
    s, w = SegmentList(iter=segs, normalize=True), SegmentList(iter=ws, normalize=True)
    assert s.asList() == list(segs) and w.asList() == list(ws)            # (the reference holds what it was handed)
    numpy.random.seed(seed)
    got = make_sampler(kind, bucket_size).sample(s, w)
    nxt = int(numpy.random.randint(0, 4294967296))
    return [int(x) for ab in got.asList() for x in ab], nxt


def in_domain():
    cases = R.in_domain()
    plan = [(name, kind, 20) for name in ("top_tiny_b1", "top_tiny_b3", "bottom", "wide_span", "frag_top")
            for kind in (R.ANNOTATOR, R.SEGMENTS)]
    plan += [("top_tiny_b1", R.BRUTE, 20), ("bottom_brute", R.BRUTE, 20)]
    out = []
    for name, kind, n in plan:
        (segs, ws), = cases[name].units
        if name == "top_tiny_b1" and kind == R.ANNOTATOR:
            n = 200
        at_T, streams = 0, []
        for seed in range(n):
            flat, nxt = reference(kind, cases[name].bucket_size, segs, ws, seed)
            assert max(flat) <= R.T
            at_T += sum(e == R.T for e in flat[1::2])
            streams.append([seed, flat, nxt])
        out.append(dict(case=name, sampler=kind, bucket_size=cases[name].bucket_size, segments=segs, workspace=ws, streams=streams))
        print("%s / %s: %d streams, %d segments end at T" % (name, R.SAMPLER_NAMES[kind], n, at_T))
    return out


def long_segments_at_the_top():
    """[(T - 80000, T - 50000), (T - 30000, T)] and three segments of about 25 000 bases"""
    T = R.T
    segs = [(T - 79900, T - 54900), (T - 54800, T - 29790), (T - 29700, T - 4680)]
    return R.Case("long_segments_at_the_top", [(segs, [(T - 80000, T - 50000), (T - 30000, T)])], 1, 0, 100, None)


def past_border():
    T = R.T
    runs = [(R.moved(R.top_tiny(1), 1, "top_tiny_one_base_past"), R.ANNOTATOR, 200),
            (R.top_tiny(1, last=(T - 1, T))._replace(name="top_tiny_last_piece_at_T"), R.ANNOTATOR, 200),
            (R.top_tiny(1)._replace(name="top_tiny_sized_for_bucket_1_run_with_3", bucket_size=3), R.ANNOTATOR, 200),
            (long_segments_at_the_top(), R.ANNOTATOR, 100)]
    out = []
    for case, kind, n in runs:
        (segs, ws), = case.units
        assert R.highest_end(case) > T
        raised = []
        for seed in range(n):
            try:
                reference(kind, case.bucket_size, segs, ws, seed)
            except Exception as e:                # noqa: BLE001 -- whatever the reference raises is what is recorded
                tb = [f for f in traceback.extract_tb(e.__traceback__) if f.filename.endswith(".pyx")]
                raised.append([seed, type(e).__name__, os.path.basename(tb[-1].filename) if tb else None,
                               tb[-1].lineno if tb else None, str(e)[:200]])
        out.append(dict(case=case.name, sampler=kind, bucket_size=case.bucket_size, segments=segs, workspace=ws, streams=n,
                        highest_end_minus_T=R.highest_end(case) - T, raised=raised))
        print("%s: the reference raised on %d of %d streams" % (case.name, len(raised), n))
    return out


if __name__ == "__main__":
    doc = dict(T=R.T, nbuckets=R.NBUCKETS, in_domain=in_domain(), past_border=past_border())
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("wrote %s: %d in-domain streams, %d past-border runs, %d bytes" % (OUT, sum(len(g["streams"]) for g in doc["in_domain"]), len(doc["past_border"]),
                                                                             os.path.getsize(OUT)))
