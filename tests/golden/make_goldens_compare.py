#!/usr/bin/env python
"""Golden tables of gat-compare, taken from the REFERENCE ITSELF -- tests/golden/compare/.

Run in the build container only, like the other make_goldens_*.py:

    bash tests/golden/build_reference.sh
    PYTHONPATH=/tmp/gatbuild python tests/golden/make_goldens_compare.py

The reference's scripts/gat-run.py and scripts/gat-compare.py run unchanged under the scratch build (no fix of the
scratch copy was needed for either).

  a.counts.tsv, b.counts.tsv   --output-counts-pattern files of two runs of 3 segment tracks x 4 annotations x 50
                               samples; they share the tracks segA, segB and the annotations t0, t1, t2 (a has segC and
                               t3, b has segD and t4 beside them)
  single.counts.tsv            one run of one segment track ("merged") x 5 annotations x 50 samples
  expected_<case>.tsv          the reference's table for the case; cases.json: {case: {"files": [...], "args": [...]}}

The inputs are tests/golden/cli/*.bed; the extra tracks are made of every other interval of two of theirs.  The
reference walks the shared annotations of two files in the order of a Python set: rows that tie in the sort key would
come out in the order of that run's string hashes.  The two-file cases are therefore ordered by `observed` (the default)
and the generator asserts that no two rows of them tie; the `--order=pvalue` case (p-values of 50 samples tie) is a
single-file one, whose pairs have a defined order.

Asserted here for every sample of every pair of every case: r = fc1 / fc2 has |log r| > 1e-9 or r == 1 -- no sample
lands within rounding of the observed value without being equal to it, so the counts below / equal to it (the p-value)
do not depend on whose logarithm is used.
"""
import collections
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "compare")
CLI = os.path.join(HERE, "cli")

import gat                                   # noqa: E402  (the reference, from PYTHONPATH)

REF = os.path.join(os.path.dirname(gat.__file__), "..", "scripts")


def read_tracks(path):
    tracks = collections.OrderedDict()
    name = None
    for line in open(path):
        if line.startswith("track"):
            name = line.split("name=")[1].strip()
            tracks[name] = []
        elif line.strip():
            tracks[name].append(line)
    return tracks


def write_tracks(path, tracks):
    with open(path, "w") as f:
        for name, lines in tracks.items():
            f.write("track name=%s\n" % name)
            f.writelines(lines)


def reference(script, args, stdout):
    env = dict(os.environ, PYTHONHASHSEED="0")
    with open(stdout, "w") as out:
        subprocess.check_call([sys.executable, os.path.join(REF, script)] + args, stdout=out, stderr=subprocess.DEVNULL, env=env)
    lines = [l for l in open(stdout) if not l.startswith("#")]
    with open(stdout, "w") as f:
        f.writelines(lines)
    return lines


def counts_file(tmp, name, segments, annotations, seed, with_tracks):
    seg, ann = os.path.join(tmp, name + "_segments.bed"), os.path.join(tmp, name + "_annotations.bed")
    write_tracks(seg, segments)
    write_tracks(ann, annotations)
    pattern = os.path.join(tmp, name + "_%s.counts.tsv")
    reference("gat-run.py", ["--segments=" + seg, "--annotations=" + ann, "--workspace=" + os.path.join(CLI, "workspace.bed"),
                             "--num-samples=50", "--random-seed=%d" % seed, "--output-counts-pattern=" + pattern,
                             "--log=" + os.path.join(tmp, "ref.log")] + (["--with-segment-tracks"] if with_tracks else []),
              os.path.join(tmp, name + ".tsv"))
    out = os.path.join(OUT, name + ".counts.tsv")
    with open(out, "w") as f:
        f.write(open(pattern % "nucleotide-overlap").read())
    return out


def check_no_sample_near_observed(files, pseudo_count):
    """|log r| > 1e-9 or r == 1 for every sample of every pair the case compares"""
    all_results = [gat.fromCounts(f) for f in files]
    if len(all_results) == 1:
        pairs = list(itertools.combinations(all_results[0], 2))
    else:
        pairs = []
        for a, b in itertools.combinations(all_results, 2):
            bb = dict(((x.track, x.annotation), x) for x in b)
            pairs += [(x, bb[(x.track, x.annotation)]) for x in a if (x.track, x.annotation) in bb]
    n = 0
    for d1, d2 in pairs:
        r = (d1.observed / (d1.samples + pseudo_count) + 0.0001) / (d2.observed / (d2.samples + pseudo_count) + 0.0001)
        assert numpy.all(numpy.isfinite(r))
        assert numpy.all((numpy.abs(numpy.log(r)) > 1e-9) | (r == 1)), (d1.track, d1.annotation, d2.annotation)
        n += len(r)
    return len(pairs), n


def main():
    os.makedirs(OUT, exist_ok=True)
    S, A = read_tracks(os.path.join(CLI, "segments.bed")), read_tracks(os.path.join(CLI, "annotations.bed"))
    segC = sorted(S["segA"][::2] + S["segB"][1::3], key=lambda l: (l.split("\t")[0], int(l.split("\t")[1])))
    segD = sorted(S["segB"][::2] + S["segA"][1::3], key=lambda l: (l.split("\t")[0], int(l.split("\t")[1])))
    t3 = sorted(A["t0"][::2] + A["t1"][::2], key=lambda l: (l.split("\t")[0], int(l.split("\t")[1])))
    t4 = sorted(A["t2"][::2] + A["t1"][1::2], key=lambda l: (l.split("\t")[0], int(l.split("\t")[1])))
    od = collections.OrderedDict
    with tempfile.TemporaryDirectory() as tmp:
        counts_file(tmp, "a", od([("segA", S["segA"]), ("segB", S["segB"]), ("segC", segC)]),
                    od([("t0", A["t0"]), ("t1", A["t1"]), ("t2", A["t2"]), ("t3", t3)]), 31, True)
        counts_file(tmp, "b", od([("segA", S["segA"]), ("segB", S["segB"]), ("segD", segD)]),
                    od([("t0", A["t0"]), ("t1", A["t1"]), ("t2", A["t2"]), ("t4", t4)]), 32, True)
        counts_file(tmp, "single", S, od([("t0", A["t0"]), ("t1", A["t1"]), ("t2", A["t2"]), ("t3", t3), ("t4", t4)]), 33, False)
    cases = od([
        ("two_files", dict(files=["a.counts.tsv", "b.counts.tsv"], args=[])),
        ("single_file", dict(files=["single.counts.tsv"], args=[])),
        ("pseudo_count_order_pvalue", dict(files=["single.counts.tsv"], args=["--pseudo-count=0.5", "--order=pvalue"])),
        ("storey", dict(files=["a.counts.tsv", "b.counts.tsv"], args=["--qvalue-method=storey"])),
    ])
    for name, case in cases.items():
        files = [os.path.join(OUT, f) for f in case["files"]]
        pc = [float(x.split("=")[1]) for x in case["args"] if x.startswith("--pseudo-count")]
        n_pairs, n = check_no_sample_near_observed(files, pc[0] if pc else 1.0)
        lines = reference("gat-compare.py", case["args"] + files, os.path.join(OUT, "expected_%s.tsv" % name))
        assert len(lines) == n_pairs + 1
        if len(files) > 1:
            observed = [l.split("\t")[2] for l in lines[1:]]
            assert len(set(observed)) == len(observed), "rows tie in the sort key: their order is a set's"
        print("%s: %d pairs, %d samples checked, %d rows" % (name, n_pairs, n, len(lines) - 1))
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(cases, f, indent=1)


if __name__ == "__main__":
    main()
