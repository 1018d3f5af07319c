#!/usr/bin/env python
"""Golden vectors of SamplerGlobalPermutation (gat/Engine.pyx:1234-1386), taken from the REFERENCE ITSELF --
tests/golden/permutation/.

Run in the build container only, like make_goldens.py (whose helpers it imports, unchanged):

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_goldens_permutation.py

  kat.json       single-unit known answers: random.seed(seed), then SamplerGlobalPermutation().sample(segments,
                 workspace) -- the list, and the next random.getrandbits(32) (what the sample consumed);
                 {"shapes": [[segments, workspace]], "cases": [[shape, seed, flat list, next]]}.  Hand-made shapes (filter
                 semantics, overhangs, bridged gaps, adjacent workspace pieces, n = 1, free = 0, free + 1 a power of two,
                 a segment across the wrap point, coordinates near 2^31) and random ones.
  cli/           the reference's gat-run.py -m global-permutation under the per-unit stream patch
                 (make_goldens.reference_cli), the re-seeding sampler seeding Python's random with the same value, on
                 tests/golden/cli/*.bed: expected_<case>.tsv and cases.json
"""
import collections
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as MG                    # noqa: E402  (imports the reference from PYTHONPATH)
import gat                                   # noqa: E402
import gat.Engine as Engine                  # noqa: E402
from gat.SegmentList import SegmentList      # noqa: E402

OUT = os.path.join(HERE, "permutation")


class PyReseedingSampler(MG.ReseedingSampler):
    """make_goldens.ReseedingSampler that also seeds Python's random (what SamplerGlobalPermutation draws from) with the
    unit's value."""

    def sample(self, segments, workspace):
        u = self.unit_of[id(segments)]
        random.seed((self.base_seed + self.sample_id * self.n_units + u) & 0xFFFFFFFF)
        return super().sample(segments, workspace)


def rand_norm(r, n, span, maxlen, start=0):
    pts = sorted(r.sample(range(start, span), 2 * n))
    out = []
    for i in range(n):
        s, e = pts[2 * i], min(pts[2 * i + 1], pts[2 * i] + maxlen)
        if e > s:
            out.append((s, e))
    return out


def kats():
    r = random.Random(20261)
    big = 2 ** 31 - 1
    shapes = [
        ([(10, 20)], [(100, 200)]),                                   # no working segment: empty, nothing drawn
        ([(90, 100), (200, 210)], [(100, 200)]),                      # segments only touching the workspace
        ([(5, 30), (150, 260)], [(20, 100), (120, 200)]),             # overhanging both ends of pieces
        ([(90, 130)], [(0, 100), (120, 300)]),                        # a segment bridging a gap
        ([(10, 20), (55, 60)], [(0, 30), (30, 50), (50, 80)]),        # adjacent pieces: merge(0) unites them
        ([(30, 45)], [(0, 100)]),                                     # n = 1
        ([(0, 40), (40, 100)], [(0, 100)]),                           # free = 0
        ([(0, 10), (20, 30)], [(0, 35), (40, 45)]),                   # free = 20 ... (and below: free + 1 = 2^m)
        ([(0, 10), (20, 31)], [(0, 40), (50, 62)]),                   # free + 1 = 32
        ([(0, 1), (5, 8)], [(0, 4), (6, 12)]),                        # free + 1 = 8
        ([(0, 900)], [(0, 1000)]),                                    # one long segment: crosses the wrap point often
        ([(10, 300), (400, 700)], [(0, 350), (380, 720), (800, 810)]),   # long segments, few free bases: wraps
        ([(big - 1000, big - 10)], [(big - 2000, big - 1)]),          # near 2^31
        ([(5, 100), (2 ** 30, 2 ** 30 + 50)], [(0, big - 1)]),        # free + 1 ~ 2^31: k = 31
        ([(0, 2)], [(0, 2 ** 30 + 1)]),                               # free + 1 = 2^30: a power of two, k = 31
        ([(1, 2)], [(0, 2 ** 30 + 2)]),                               # free + 1 = 2^30 + 1: about half rejected
    ]
    for kind in range(14):
        span = r.choice([200, 1000, 5000])
        segs = rand_norm(r, r.randint(1, 14), span, r.choice([3, 30, 300]))
        if kind % 3 == 0:
            ws = rand_norm(r, 40, span + 100, 5)                       # fragmented
        else:
            ws = rand_norm(r, r.randint(1, 8), span + 100, r.choice([50, 2000]))
        shapes.append((segs, ws))
    cases = []
    for i, (segs, ws) in enumerate(shapes):
        seeds = [0, 1, 2 ** 32 - 1, 7 + i, r.randrange(2 ** 32)]
        if i < 16:
            seeds += [r.randrange(2 ** 32) for _ in range(5)]
        for seed in seeds:
            random.seed(seed)
            got = Engine.SamplerGlobalPermutation().sample(SegmentList(iter=segs, normalize=True),
                                                           SegmentList(iter=ws, normalize=True))
            nxt = random.getrandbits(32)
            cases.append([i, seed, [int(x) for ab in got for x in ab], nxt])
    # random shapes, one seed each
    for _ in range(300):
        span = r.choice([100, 1000, 20000])
        segs = rand_norm(r, r.randint(1, 10), span, r.choice([2, 20, 400]))
        ws = rand_norm(r, r.randint(1, 12), span + 50, r.choice([3, 40, 5000]))
        if not segs or not ws:
            continue
        shapes.append((segs, ws))
        seed = r.randrange(2 ** 32)
        random.seed(seed)
        got = Engine.SamplerGlobalPermutation().sample(SegmentList(iter=segs, normalize=True),
                                                       SegmentList(iter=ws, normalize=True))
        cases.append([len(shapes) - 1, seed, [int(x) for ab in got for x in ab], random.getrandbits(32)])
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(dict(shapes=shapes, cases=cases), f, separators=(",", ":"))
    print("kat: %d shapes, %d cases" % (len(shapes), len(cases)))


def cli():
    cli_in = os.path.join(HERE, "cli")
    out_dir = os.path.join(OUT, "cli")
    os.makedirs(out_dir, exist_ok=True)
    cases = collections.OrderedDict([
        ("plain", ["--num-samples=40", "--random-seed=7", "--sampler=global-permutation"]),
        ("isochores", ["--num-samples=30", "--random-seed=42", "--sampler=global-permutation",
                       "--isochores=isochores.bed", "--counter=segment-overlap"]),
        ("segment_tracks", ["--num-samples=25", "--random-seed=43", "--sampler=global-permutation",
                            "--with-segment-tracks", "--order=track"]),
        ("conditional", ["--num-samples=20", "--random-seed=44", "--sampler=global-permutation",
                         "--conditional=segment-centered", "--conditional-expansion=3", "--order=annotation"]),
    ])
    MG.ReseedingSampler = PyReseedingSampler                     # (reference_cli builds its sampler from this name)
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
