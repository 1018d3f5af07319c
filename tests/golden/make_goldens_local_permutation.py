#!/usr/bin/env python
"""Golden vectors of SamplerLocalPermutation (gat/Engine.pyx:1117-1229), taken from the REFERENCE ITSELF --
tests/golden/local_permutation/.

Run in the build container only, like make_goldens_permutation.py (whose re-seeding sampler and shape helper it uses;
make_goldens.py is imported unchanged):

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_goldens_local_permutation.py 2> /dev/null

(stderr: the reference prints "Exception ignored ... minimum from non-normalized list" twice per workspace piece -- see
tests/local_permutation_model.py.)

  kat.json       single-unit known answers: random.seed(seed), then SamplerLocalPermutation().sample(segments,
                 workspace) -- the list, and the next random.getrandbits(32) (what the sample consumed);
                 {"shapes": [[segments, workspace]], "cases": [[shape, seed, flat list, next]]}.  Where the reference
                 raises, the flat list is the exception's class name and next is null.
  cli/           the reference's gat-run.py -m local-permutation under the per-unit stream patch
                 (make_goldens.reference_cli) on tests/golden/cli/*.bed: expected_<case>.tsv and cases.json
"""
import collections
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as MG                    # noqa: E402  (imports the reference from PYTHONPATH)
import make_goldens_permutation as MP        # noqa: E402
import gat                                   # noqa: E402
import gat.Engine as Engine                  # noqa: E402
from gat.SegmentList import SegmentList      # noqa: E402

OUT = os.path.join(HERE, "local_permutation")
rand_norm = MP.rand_norm


def reference(segs, ws, seed):
    random.seed(seed)
    try:
        got = Engine.SamplerLocalPermutation().sample(SegmentList(iter=segs, normalize=True),
                                                      SegmentList(iter=ws, normalize=True))
    except Exception as e:                    # noqa: BLE001 -- whatever the reference raises is what is recorded
        return type(e).__name__, None
    return [int(x) for ab in got for x in ab], random.getrandbits(32)


def kats():
    r = random.Random(20268)
    big = 2 ** 31 - 1
    many = [(100 + 10 * i, 103 + 10 * i + i % 5) for i in range(90)]          # 90 segments in one piece
    shapes = [
        ([(500, 510)], [(100, 200)]),                                 # every segment beyond the workspace: empty, no draw
        ([(10, 20)], [(100, 200)]),                                   # output although filter() is empty: the segment before the piece
        ([(10, 20)], [(0, 5), (100, 200), (300, 310)]),               # an idle piece, then active ones; the segment works for two
        ([(100, 110), (150, 160)], [(90, 200), (300, 400)]),          # piece 2 takes the last segment only
        ([(10, 20), (200, 230)], [(50, 200), (200, 260)]),            # adjacent pieces; a segment starting AT a piece's end is working
        ([(50, 60)], [(50, 100)]),                                    # segment starting at the piece's start
        ([(30, 45)], [(0, 100)]),                                     # n = 1
        ([(0, 40), (40, 100)], [(0, 100)]),                           # free = 0: every draw _randbelow(1)
        ([(0, 40), (40, 101)], [(0, 100)]),                           # free < 0: the reference raises
        ([(0, 10), (20, 31)], [(5, 52)]),                             # free + 1 = 32
        ([(0, 1), (5, 8)], [(0, 11)]),                                # free + 1 = 8
        ([(0, 3)], [(1, 36)]),                                        # free + 1 = 34: just above 32, about half rejected
        ([(0, 900)], [(0, 1000)]),                                    # one long segment: wraps often
        ([(10, 300), (400, 700)], [(0, 650)]),                        # long segments, few free bases: wraps, ends on work_end
        ([(0, 5), (7, 12)], [(0, 12)]),                               # free = 2: starts and ends on work_end
        (many, [(0, 2000)]),                                          # n > 64 in one piece
        (many, [(0, 150), (160, 170), (400, 1200), (1300, 1301)]),    # ... and spread over pieces
        ([(big - 1000, big - 10)], [(big - 2000, big - 1)]),          # near 2^31: OverflowError for about half the seeds
        ([(5, 100), (2 ** 30, 2 ** 30 + 50)], [(0, big - 1)]),        # free + 1 ~ 2^31: k = 31
        ([(0, 2)], [(0, 2 ** 30 + 1)]),                               # free + 1 = 2^30: a power of two
        ([(1, 2)], [(0, 2 ** 30 + 1)]),                               # free + 1 = 2^30 + 1: about half rejected
    ]
    for kind in range(14):
        span = r.choice([200, 1000, 5000])
        segs = rand_norm(r, r.randint(1, 14), span, r.choice([3, 30, 300]), start=r.choice([0, span // 2]))
        if kind % 3 == 0:
            ws = rand_norm(r, 40, span + 100, 5)                       # fragmented
        else:
            ws = rand_norm(r, r.randint(1, 8), span + 100, r.choice([50, 2000]))
        shapes.append((segs, ws))
    n_fixed = len(shapes)
    cases = []
    for i, (segs, ws) in enumerate(shapes):
        seeds = [0, 1, 2 ** 32 - 1, 7 + i, r.randrange(2 ** 32)]
        if i < n_fixed - 14:
            seeds += [r.randrange(2 ** 32) for _ in range(5)]
        for seed in seeds:
            flat, nxt = reference(segs, ws, seed)
            cases.append([i, seed, flat, nxt])
    # random shapes, one seed each; every third one fragmented
    for k in range(300):
        span = r.choice([100, 1000, 20000])
        segs = rand_norm(r, r.randint(1, 10), span, r.choice([2, 20, 400]), start=r.choice([0, 0, span // 3]))
        if k % 3 == 0:
            ws = rand_norm(r, r.randint(20, 60), span + 50, r.choice([2, 6]))
        else:
            ws = rand_norm(r, r.randint(1, 12), span + 50, r.choice([3, 40, 5000]))
        if not segs or not ws:
            continue
        shapes.append((segs, ws))
        seed = r.randrange(2 ** 32)
        flat, nxt = reference(segs, ws, seed)
        cases.append([len(shapes) - 1, seed, flat, nxt])
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(dict(shapes=shapes, cases=cases), f, separators=(",", ":"))
    print("kat: %d shapes, %d cases, %d raised" % (len(shapes), len(cases), sum(isinstance(c[2], str) for c in cases)))


def cli():
    cli_in = os.path.join(HERE, "cli")
    out_dir = os.path.join(OUT, "cli")
    os.makedirs(out_dir, exist_ok=True)
    cases = collections.OrderedDict([
        ("plain", ["--num-samples=40", "--random-seed=7", "--sampler=local-permutation"]),
        ("isochores", ["--num-samples=30", "--random-seed=42", "--sampler=local-permutation",
                       "--isochores=isochores.bed", "--counter=segment-overlap"]),
        ("segment_tracks", ["--num-samples=25", "--random-seed=43", "--sampler=local-permutation",
                            "--with-segment-tracks", "--order=track"]),
        ("conditional", ["--num-samples=20", "--random-seed=44", "--sampler=local-permutation",
                         "--conditional=segment-centered", "--conditional-expansion=3", "--order=annotation"]),
    ])
    MG.ReseedingSampler = MP.PyReseedingSampler                  # (reference_cli builds its sampler from this name)
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
