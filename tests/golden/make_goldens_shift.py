#!/usr/bin/env python
"""Golden vectors of SamplerShift (gat/Engine.pyx:998-1111), taken from the REFERENCE ITSELF -- tests/golden/shift/.

Run in the build container only, like make_goldens.py (whose helpers it imports, unchanged):

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_goldens_shift.py

  kat.json       single-unit known answers: numpy.random.seed(seed), then SamplerShift(radius, extension).sample(
                 segments, workspace) -- the list, and the next randint(0, 2**31) (what the sample consumed);
                 {"shapes": [[segments, workspace]], "cases": [[shape, radius, extension, seed, flat list, next]]}.  Segments
                 near 0, windows smaller than the segment, fragmented and empty windows, windows of one base.
  cli/           the reference's gat-run.py -m shift under the per-unit stream patch (make_goldens.reference_cli) on
                 tests/golden/cli/*.bed: expected_<case>.tsv and cases.json
"""
import collections
import json
import os
import random
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as MG                    # noqa: E402  (imports the reference from PYTHONPATH)
import gat                                   # noqa: E402
import gat.Engine as Engine                  # noqa: E402
from gat.SegmentList import SegmentList      # noqa: E402

OUT = os.path.join(HERE, "shift")


def rand_norm(r, n, span, maxlen):
    pts = sorted(r.sample(range(0, span), 2 * n))
    out = []
    for i in range(n):
        s, e = pts[2 * i], min(pts[2 * i + 1], pts[2 * i] + maxlen)
        if e > s:
            out.append((s, e))
    return out


def kats():
    r = random.Random(20260)
    # hand-made: near 0 (start - length wraps), one-base windows, segments longer than their window, gapped workspace
    shapes = [([(10, 50)], [(0, 1000)]),
              ([(0, 3), (5, 6)], [(0, 8)]),
              ([(100, 400)], [(150, 160), (170, 171), (390, 395)]),
              ([(1000, 1001), (2000, 2100)], [(990, 1000), (1001, 1002), (2000, 2001)]),
              ([(20, 30), (40, 45), (300, 330)], [(0, 25), (28, 29), (33, 60), (200, 400)])]
    for fragmented in (True, False, False):
        span = r.choice([200, 1000])
        segs = rand_norm(r, r.randint(2, 6), span, r.choice([5, 50]))
        ws = rand_norm(r, 30, span + 100, 3) if fragmented else rand_norm(r, r.randint(2, 8), span + 100, 2000)
        shapes.append((segs, ws))
    # params: radius in {0, 0.5, 1, 2, 3.7} (extension 0), extension in {1, 7, 200, 500.0} (radius 2); 5 seeds each
    params = [(0, 0), (0.5, 0), (1, 0), (2, 0), (3.7, 0), (2, 1), (2, 7), (2, 200), (2, 500.0)]
    cases = []
    for i, (segs, ws) in enumerate(shapes):
        for radius, extension in params:
            for seed in (1, 2, 3 + i, 12345, 2 ** 32 - 1 - i):
                numpy.random.seed(seed)
                got = Engine.SamplerShift(radius=radius, extension=extension).sample(
                    SegmentList(iter=segs, normalize=True), SegmentList(iter=ws, normalize=True))
                nxt = int(numpy.random.randint(0, 2 ** 31))
                # [shape, radius, extension, seed, the sample's coordinates flattened, next draw]
                cases.append([i, radius, extension, seed, [int(x) for ab in got for x in ab], nxt])
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(dict(shapes=shapes, cases=cases), f, separators=(",", ":"))
    print("kat: %d cases" % len(cases))


def cli():
    cli_in = os.path.join(HERE, "cli")
    out_dir = os.path.join(OUT, "cli")
    os.makedirs(out_dir, exist_ok=True)
    cases = collections.OrderedDict([
        ("plain", ["--num-samples=40", "--random-seed=31", "--sampler=shift"]),
        ("isochores", ["--num-samples=30", "--random-seed=32", "--sampler=shift", "--isochores=isochores.bed",
                       "--counter=segment-overlap"]),
        ("extension", ["--num-samples=30", "--random-seed=33", "--sampler=shift", "--shift-extension=500"]),
        ("expansion", ["--num-samples=30", "--random-seed=34", "--sampler=shift", "--shift-expansion=0.5"]),
        ("segment_tracks", ["--num-samples=25", "--random-seed=35", "--sampler=shift", "--with-segment-tracks",
                            "--order=track"]),
        ("conditional", ["--num-samples=20", "--random-seed=36", "--sampler=shift", "--conditional=segment-centered",
                         "--conditional-expansion=3", "--order=annotation"]),
    ])
    mod, state, patched, original = MG.reference_cli()
    gat.computeSample = patched
    try:
        for name, extra in cases.items():
            out = os.path.join(out_dir, "expected_%s.tsv" % name)
            args = [x.replace("--isochores=", "--isochores=%s%s" % (cli_in, os.sep)) for x in extra]
            argv = ["gat-run.py", "--segments=%s" % os.path.join(cli_in, "segments.bed"),
                    "--annotations=%s" % os.path.join(cli_in, "annotations.bed"),
                    "--workspace=%s" % os.path.join(cli_in, "workspace.bed"),
                    "--stdout=%s" % out, "--log=%s" % os.path.join(out_dir, "ref.log")] + args
            seed = int([x for x in extra if x.startswith("--random-seed")][0].split("=")[1])
            ns = int([x for x in extra if x.startswith("--num-samples")][0].split("=")[1])
            state.update(track=None, base=seed, n_units=0, sampler=None, num_samples=ns)
            mod.main(argv)
            lines = [l for l in open(out) if not l.startswith("#")]
            with open(out, "w") as f:
                f.writelines(lines)
            print("cli %s: %d rows" % (name, len(lines) - 1))
    finally:
        gat.computeSample = original
    if os.path.exists(os.path.join(out_dir, "ref.log")):
        os.remove(os.path.join(out_dir, "ref.log"))
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(cases, f)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    kats()
    cli()
