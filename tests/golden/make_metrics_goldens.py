#!/usr/bin/env python
"""Golden vectors of --output-stats=segment_metrics / sample_metrics (gat/IO.py:331-454, SegmentsSummary / outputMetrics),
taken from the REFERENCE ITSELF -- tests/golden/metrics/.

Run in the build container only, like make_goldens.py (whose helpers it imports, unchanged):

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_metrics_goldens.py

In the reference both options die in Stats.Summary with a TypeError (gat/Stats.py:375-376: a Python-2 integer division used
as a list index).  On the SCRATCH COPY build_reference.sh made -- never on the reference -- this script applies the
substitutions that let Stats.Summary run under Python 3, and nothing else:

    gat/Stats.py:375    self.q1 = n[len(n) / 4]        ->  self.q1 = n[len(n) // 4]
    gat/Stats.py:376    self.q3 = n[len(n) * 3 / 4]    ->  self.q3 = n[len(n) * 3 // 4]

(`reduce` is imported there already: from functools import reduce.)  Neither touches arithmetic: `//` is what `/` meant
between two ints when the line was written.

  kat.json       explicit (list, workspace) pairs: {"cases": [{"name", "segments", "workspace", the attributes of
                 SegmentsSummary.update}], "groups": [{"keys": [case names], "text": what outputMetrics writes for the
                 dictionary of those cases}]}.  Geometry: empty list, empty workspace, a segment equal to a piece, touching
                 without overlap on either side, over two adjacent pieces, over two pieces with a gap, over all pieces,
                 before the first and behind the last piece, coordinates at 2^31 - 1, random lists.
  cli/           the reference's gat-run.py under the per-unit stream patch (make_goldens.reference_cli) on
                 tests/golden/cli/*.bed, 20 samples: expected_<case>.tsv, expected_<case>.segment_metrics,
                 expected_<case>.sample_metrics and cases.json -- `plain` and `tracks` (--with-segment-tracks) with both
                 options, `isochores` with segment_metrics alone (the reference looks a contig-level sample up in the
                 isochore-keyed workspace: its sample_metrics with isochores say nothing and are not pinned)
"""
import collections
import io
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SUBSTITUTIONS = (("self.q1 = n[len(n) / 4]", "self.q1 = n[len(n) // 4]"),
                 ("self.q3 = n[len(n) * 3 / 4]", "self.q3 = n[len(n) * 3 // 4]"))


def patch_scratch_copy():
    """the two substitutions, on the gat/Stats.py that PYTHONPATH leads to; refuses anything but a scratch copy"""
    for d in sys.path:
        path = os.path.join(d, "gat", "Stats.py")
        if d and os.path.exists(path):
            break
    else:
        raise SystemExit("no gat/Stats.py on PYTHONPATH: run tests/golden/build_reference.sh first")
    if not os.path.exists(os.path.join(os.path.dirname(path), "..", "setup_probe.py")):
        raise SystemExit("%s is not the scratch copy of build_reference.sh" % path)
    text = open(path).read()
    for old, new in SUBSTITUTIONS:
        assert (old in text) != (new in text), "gat/Stats.py: expected exactly one of %r / %r" % (old, new)
        text = text.replace(old, new)
    with open(path, "w") as f:
        f.write(text)


patch_scratch_copy()

import make_goldens as MG                    # noqa: E402  (imports the reference from PYTHONPATH)
import gat                                   # noqa: E402
import gat.IO as IO                          # noqa: E402
from gat.SegmentList import SegmentList      # noqa: E402

OUT = os.path.join(HERE, "metrics")
TOP = 2 ** 31 - 1
INT_ATTRIBUTES = ("all_segments", "all_nucleotides", "segments_overlapping_workspace", "nucleotides_overlapping_workspace",
                  "segments_outside_workspace", "nucleotides_outside_workspace", "truncated_segments", "truncated_nucleotides")
FLOAT_ATTRIBUTES = ("density_workspace", "proportion_truncated_segments", "proportion_extending_nucleotides")


def rand_lists(r, n, span, maxlen):
    """a sorted, disjoint list of up to n segments; about a third of its neighbours adjacent"""
    out, pos = [], r.randint(0, span // 4)
    for _ in range(n):
        ln = r.randint(1, maxlen)
        out.append((pos, pos + ln))
        pos += ln + (0 if r.random() < 0.35 else r.randint(1, span // max(1, n)))
    return out


def kat_shapes():
    ws3 = [(100, 200), (200, 300), (350, 400)]               # two adjacent pieces, then a gap
    shapes = collections.OrderedDict([
        ("empty_list", ([], ws3)),
        ("empty_workspace", ([(10, 20), (30, 40)], [])),
        ("both_empty", ([], [])),
        ("equal_to_a_piece", ([(200, 300)], ws3)),
        ("ends_at_piece_start", ([(50, 100)], ws3)),
        ("starts_at_piece_end", ([(300, 350)], ws3)),
        ("touching_both_sides", ([(300, 350)], [(100, 300), (350, 400)])),
        ("over_two_adjacent", ([(150, 250)], ws3)),
        ("over_two_with_gap", ([(250, 380)], ws3)),
        ("inside_the_gap_and_beyond", ([(290, 360)], ws3)),
        ("over_all_pieces", ([(50, 500)], ws3)),
        ("exactly_all_pieces", ([(100, 400)], ws3)),
        ("before_first", ([(0, 10), (20, 99)], ws3)),
        ("after_last", ([(400, 410), (1000, 2000)], ws3)),
        ("before_inside_after", ([(0, 10), (90, 110), (120, 130), (190, 210), (299, 351), (399, 401), (500, 600)], ws3)),
        ("adjacent_segments", ([(100, 150), (150, 200), (200, 260), (260, 300), (300, 350), (350, 410)], ws3)),
        ("top_coordinates", ([(TOP - 1000, TOP - 500), (TOP - 400, TOP)], [(TOP - 700, TOP - 450), (TOP - 450, TOP - 100), (TOP - 50, TOP)])),
        ("top_outside", ([(TOP - 10, TOP)], [(0, 5)])),
        ("one_base", ([(5, 6)], [(5, 6)])),
        ("many_small_pieces", ([(0, 1000)], [(10 * i, 10 * i + (10 if i % 3 == 0 else 4)) for i in range(90)])),
    ])
    r = random.Random(20261018)
    for i in range(12):
        span = r.choice([300, 5000, 200000])
        segs = rand_lists(r, r.choice([1, 5, 40, 130]), span, r.choice([3, 60, 700]))
        ws = rand_lists(r, r.choice([1, 2, 9, 70]), span, r.choice([5, 200, 3000]))
        shapes["random_%02d" % i] = (segs, ws)
    return shapes


def kats():
    shapes = kat_shapes()
    cases = []
    for name, (segs, ws) in shapes.items():
        s = IO.SegmentsSummary()
        s.update(SegmentList(iter=segs, normalize=True), SegmentList(iter=ws, normalize=True))
        case = collections.OrderedDict(name=name, segments=segs, workspace=ws)
        for a in INT_ATTRIBUTES:
            case[a] = int(getattr(s, a))
        for a in FLOAT_ATTRIBUTES:
            case[a] = float(getattr(s, a))
        cases.append(case)
    names = list(shapes)
    groups = []
    for keys in ([names[0]], names[:3], names[3:12], names[12:20], names[20:], names, []):
        segments = collections.OrderedDict((k, SegmentList(iter=shapes[k][0], normalize=True)) for k in keys)
        workspace = dict((k, SegmentList(iter=shapes[k][1], normalize=True)) for k in keys)
        out = io.StringIO()
        IO.outputMetrics(out, segments, workspace, "kat", "group%d" % len(groups))
        groups.append(collections.OrderedDict(keys=keys, text=out.getvalue()))
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(collections.OrderedDict(cases=cases, groups=groups), f, indent=0, separators=(",", ":"))
    print("kat: %d cases, %d groups" % (len(cases), len(groups)))


def cli():
    cli_in = os.path.join(HERE, "cli")
    out_dir = os.path.join(OUT, "cli")
    os.makedirs(out_dir, exist_ok=True)
    both = ["--output-stats=segment_metrics", "--output-stats=sample_metrics"]
    cases = collections.OrderedDict([
        ("plain", ["--num-samples=20", "--random-seed=51"] + both),
        ("tracks", ["--num-samples=20", "--random-seed=52", "--with-segment-tracks", "--order=track"] + both),
        ("isochores", ["--num-samples=20", "--random-seed=53", "--isochores=isochores.bed", "--output-stats=segment_metrics"]),
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
                    "--output-filename-pattern=%s" % os.path.join(out_dir, "expected_%s.%%s" % name), "--force",
                    "--stdout=%s" % out, "--log=%s" % os.path.join(out_dir, "ref.log")] + args
            seed = int([x for x in extra if x.startswith("--random-seed")][0].split("=")[1])
            ns = int([x for x in extra if x.startswith("--num-samples")][0].split("=")[1])
            state.update(track=None, base=seed, n_units=0, sampler=None, num_samples=ns)
            mod.main(argv)
            lines = [l for l in open(out) if not l.startswith("#")]
            with open(out, "w") as f:
                f.writelines(lines)
            sides = [s for s in ("segment_metrics", "sample_metrics") if "--output-stats=%s" % s in extra]
            print("cli %s: %d rows; %s" % (name, len(lines) - 1, ", ".join(
                "%s %d lines" % (s, len(open(os.path.join(out_dir, "expected_%s.%s" % (name, s))).readlines())) for s in sides)))
    finally:
        gat.computeSample = original
    if os.path.exists(os.path.join(out_dir, "ref.log")):
        os.remove(os.path.join(out_dir, "ref.log"))
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(cases, f, indent=1)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    kats()
    cli()
