#!/usr/bin/env python
"""Golden vectors of SamplerBruteForce (gat/Engine.pyx:746-871), taken from the REFERENCE ITSELF --
tests/golden/brute_force/.

Run in the build container only, like make_goldens_shift.py (make_goldens.py is imported unchanged):

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_goldens_brute_force.py 2> /dev/null

(stderr: the reference prints assertions it cannot raise.)

  kat.json       single-unit known answers: numpy.random.seed(seed), then SamplerBruteForce(*params).sample(segments,
                 workspace) -- the list, and the next numpy.random.randint(0, 2**31) (what the sample consumed);
                 {"shapes": [[segments, workspace]], "cases": [[shape, [bucket_size, nbuckets, ntries_inner,
                 ntries_outer], seed, flat list, next, "fixed" | "random"]]}.  Where the reference raises, the flat list
                 is the exception's class name and next is null.
  cli/           the reference's gat-run.py -m brute-force under the per-unit stream patch (make_goldens.reference_cli) on
                 cli/segments.bed -- tests/golden/cli/segments.bed with every length cut to 1..3, so that the runs
                 converge -- and tests/golden/cli/{annotations,workspace,isochores}.bed: expected_<case>.tsv, cases.json
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

OUT = os.path.join(HERE, "brute_force")
DEFAULT = [1, 100000, 100, 10]


def rand_norm(r, n, span, maxlen, start=0):
    pts = sorted(r.sample(range(start, start + span), 2 * n))
    out = []
    for i in range(n):
        s, e = pts[2 * i], min(pts[2 * i + 1], pts[2 * i] + maxlen)
        if e > s:
            out.append((s, e))
    return out


def reference(segs, ws, params, seed):
    numpy.random.seed(seed)
    try:
        got = Engine.SamplerBruteForce(*params).sample(SegmentList(iter=segs, normalize=True),
                                                      SegmentList(iter=ws, normalize=True))
    except Exception as e:                    # noqa: BLE001 -- whatever the reference raises is what is recorded
        return type(e).__name__, None
    return [int(x) for ab in got for x in ab], int(numpy.random.randint(0, 2 ** 31))


def kats():
    r = random.Random(20270)
    dense = [(100 + 10 * i, 100 + 10 * i + 3 + i % 5) for i in range(30)]              # 152 of the piece's 300 bases
    mid = [(1, 2)] + rand_norm(r, 70, 20000, 12, start=10)                               # 60..70 accepted, a length of 1
    long_ = [(1, 2)] + rand_norm(r, 140, 40000, 12, start=10)                            # beyond 128 accepted
    shapes = [
        (([(500, 510)], [(100, 200)]), [DEFAULT]),                                       # empty working list: no draw
        (([(130, 145)], [(100, 200)]), [DEFAULT]),                                       # one segment
        (([(0, 30), (40, 41)], [(0, 60)]), [DEFAULT]),                                   # hanging off coordinate 0
        (([(10, 40), (105, 106)], [(0, 50), (60, 70), (75, 80), (100, 140)]), [DEFAULT]),  # pieces closer than a length
        (([(10, 20), (20, 30), (30, 31)], [(0, 25), (25, 40)]), [DEFAULT]),              # segments that only touch
        ((dense, [(90, 390)]), [DEFAULT, [1, 100000, 3, 2]]),                            # dense: restarts; 3 x 2 tries
        ((dense, [(90, 390), (1000, 1100)]), [DEFAULT, [1, 100000, 3, 2]]),
        ((mid, [(0, 21000)]), [DEFAULT]),
        ((long_, [(0, 42000)]), [DEFAULT]),
        (([(10, 17), (30, 51), (60, 61), (70, 73)], [(0, 100), (150, 300)]), [[0, 100000, 100, 10], [7, 100000, 100, 10],
                                                                               [0, 4, 100, 10], [7, 2, 100, 10]]),
        # non-working segments push segments.sum() to the int32 it is assigned to: 2^31 - 996, the most a list can reach --
        # SegmentList(iter=...) does not keep a coordinate beyond 2^31 - 1 ((1000, 2**31) comes back as (1000, 20)), so no
        # list the reference can be handed sums past 2^31 - 1
        (([(10, 20), (1000, 2 ** 30), (2 ** 30 + 5, 2 ** 31 - 1)], [(0, 100)]), [DEFAULT]),
        (([(10, 20), (1000, 2 ** 30)], [(0, 100)]), [DEFAULT]),                          # ... a sum the workspace cannot hold
    ]
    flat_shapes, cases = [], []
    for i, (shape, plist) in enumerate(shapes):
        flat_shapes.append(shape)
        for params in plist:
            for seed in (0, 1, 2 ** 32 - 1, 7 + i, r.randrange(2 ** 32), r.randrange(2 ** 32)):
                flat, nxt = reference(shape[0], shape[1], params, seed)
                cases.append([i, params, seed, flat, nxt, "fixed"])
    # random small cases, one seed each
    for k in range(320):
        span = r.choice([100, 400, 3000])
        segs = rand_norm(r, r.randint(1, 12), span, r.choice([2, 6, 40]), start=r.choice([0, 0, span // 3]))
        ws = rand_norm(r, r.randint(1, 6), span + 50, r.choice([40, 300, 5000]))
        if not segs or not ws:
            continue
        params = r.choice([DEFAULT, DEFAULT, [0, 100000, 100, 10], [3, 100000, 50, 4]])
        flat_shapes.append((segs, ws))
        seed = r.randrange(2 ** 32)
        flat, nxt = reference(segs, ws, params, seed)
        cases.append([len(flat_shapes) - 1, params, seed, flat, nxt, "random"])
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(dict(shapes=flat_shapes, cases=cases), f, separators=(",", ":"))
    rnd = [c for c in cases if c[5] == "random"]
    print("kat: %d shapes, %d cases (%d random), raised: %d (%d random), longest list %d" % (
        len(flat_shapes), len(cases), len(rnd), sum(isinstance(c[3], str) for c in cases),
        sum(isinstance(c[3], str) for c in rnd), max(len(c[3]) // 2 for c in cases if not isinstance(c[3], str))))


def cli_segments(cli_in, out_dir):
    """tests/golden/cli/segments.bed with every segment cut to a length of 1..3 (track lines kept)"""
    path = os.path.join(out_dir, "segments.bed")
    with open(path, "w") as f:
        for line in open(os.path.join(cli_in, "segments.bed")):
            t = line.rstrip("\n").split("\t")
            if len(t) >= 3 and t[1].isdigit():
                s, e = int(t[1]), int(t[2])
                t[2] = str(s + 1 + (e - s - 1) % 3)
                line = "\t".join(t) + "\n"
            f.write(line)
    return path


def cli():
    cli_in = os.path.join(HERE, "cli")
    out_dir = os.path.join(OUT, "cli")
    os.makedirs(out_dir, exist_ok=True)
    segments = cli_segments(cli_in, out_dir)
    cases = collections.OrderedDict([
        ("plain", ["--num-samples=40", "--random-seed=51", "--sampler=brute-force"]),
        ("isochores", ["--num-samples=30", "--random-seed=52", "--sampler=brute-force", "--isochores=isochores.bed",
                       "--counter=segment-overlap"]),
        ("segment_tracks", ["--num-samples=25", "--random-seed=53", "--sampler=brute-force", "--with-segment-tracks",
                            "--order=track"]),
        ("conditional", ["--num-samples=20", "--random-seed=54", "--sampler=brute-force", "--conditional=segment-centered",
                         "--conditional-expansion=3", "--order=annotation"]),
    ])
    mod, state, patched, original = MG.reference_cli()
    gat.computeSample = patched
    try:
        for name, extra in cases.items():
            out = os.path.join(out_dir, "expected_%s.tsv" % name)
            args = [x.replace("--isochores=", "--isochores=%s%s" % (cli_in, os.sep)) for x in extra]
            argv = ["gat-run.py", "--segments=%s" % segments,
                    "--annotations=%s" % os.path.join(cli_in, "annotations.bed"),
                    "--workspace=%s" % os.path.join(cli_in, "workspace.bed"),
                    "--stdout=%s" % out, "--log=%s" % os.path.join(out_dir, "ref.log")] + args
            seed = int([x for x in extra if x.startswith("--random-seed")][0].split("=")[1])
            ns = int([x for x in extra if x.startswith("--num-samples")][0].split("=")[1])
            state.update(track=None, base=seed, n_units=0, sampler=None, num_samples=ns)
            mod.main(argv)                     # (a run that does not converge dies here with the reference's ValueError)
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
