"""--output-stats=segment_metrics / sample_metrics: how the input segments and every sample sit in the workspace.

The reference's quality check of a randomisation (gat/IO.py:331-454, SegmentsSummary / outputMetrics; called from
computeSample, gat/__init__.py:565-576, and from run, :913-925): per key of a dictionary of segment lists ten attributes --
segments and bases, how many of them the workspace holds, how many pieces and bases stick out, the density -- and per
attribute one row `track, section, attribute, Summary(values over the keys)`.  In the reference both options die in
Stats.Summary (gat/Stats.py:375, a Python-2 integer division used as a list index); what they compute is plain, and is
what this module writes.

The ten attributes follow from eight exact integer sums per (list, workspace) that the device forms where the lists are
(k_metrics: gat_list_metrics for the input segments, gat_sample_metrics for the samples; include/gat_mi355.h has the
definitions).  For sorted, disjoint lists they equal the reference's filter / intersect / subtract -- including what its
subtract leaves out: the merge-join ends with the last piece of the intersection, so segments behind the last one that
touches the workspace are missing from truncated_segments / truncated_nucleotides (tail_n / tail_bases); for the lists of
SamplerSegments without isochore keys -- neither sorted nor disjoint -- the per-segment form is the definition and
overlapping segments count with their multiplicity, as in gat-coverage.  All sums are 64-bit (the reference's Position
accumulator wraps at 2^32).

Isochores: the reference looks a contig-level sample up in the isochore-keyed workspace, finds nothing, and reports every
sample as wholly outside.  Here a contig's sample is measured against that contig's workspace, the union of its isochore
pieces (problem.from_isochores, as coverage.py does).

Under an initialised torch.distributed process group rank 0 computes and writes, all samples, without sharding.
"""
import functools

import numpy as np

from . import intervals as iv
from . import problem

WORDS = ("n", "bases", "pairs", "inter", "touched", "outside_pieces", "tail_n", "tail_bases")
# the rows of one outputMetrics call, in the order of gat/IO.py:440-449
ATTRIBUTES = ("all_segments", "all_nucleotides", "segments_overlapping_workspace", "nucleotides_overlapping_workspace",
              "nucleotides_outside_workspace", "truncated_segments", "truncated_nucleotides", "density_workspace",
              "proportion_truncated_segments", "proportion_extending_nucleotides")
FIELDS = ("nval", "min", "max", "mean", "median", "stddev", "sum", "q1", "q3")          # Stats.Summary.fields
HEADER = "track\tsection\tmetric\t%s\n" % "\t".join(FIELDS)
SECTIONS = ("segment_metrics", "sample_metrics")


def attributes(words, workspace_bases):
    """the ten attributes (ATTRIBUTES order) of lists whose eight sums are words[..., 8] in workspaces of workspace_bases[...]
    bases: a list of ten arrays, int64 for the counts and float64 for the three ratios (0 where the reference leaves its 0)"""
    words = np.asarray(words, dtype=np.int64)
    size = np.asarray(workspace_bases, dtype=np.int64)
    n, bases, pairs, inter, touched, pieces, tail_n, tail_bases = (words[..., k] for k in range(8))
    out_bases = bases - inter
    cut_n, cut_bases = pieces - tail_n, out_bases - tail_bases          # len / sum of segments.subtract(intersection)
    with np.errstate(divide="ignore", invalid="ignore"):
        density = np.where(size > 0, inter.astype(np.float64) / size, 0.0)
        prop_segments = np.where(pairs > 0, cut_n.astype(np.float64) / pairs, 0.0)
        prop_bases = np.where(pairs > 0, cut_bases.astype(np.float64) / touched, 0.0)
    return [n, bases, pairs, inter, out_bases, cut_n, cut_bases, density, prop_segments, prop_bases]


def summary(values):
    """Stats.Summary(values) as written for Python 2 (gat/Stats.py:338-415): the nine fields as text.  Sorted values,
    q1 = v[len // 4], q3 = v[len * 3 // 4], population standard deviation, every field but nval with %6.4f."""
    n = sorted(x for x in values if x is not None)
    if not n:
        return "\t".join(["0"] + ["%6.4f" % 0] * 8)
    q1, q3 = n[len(n) // 4], n[len(n) * 3 // 4]
    fields = (min(n), max(n), np.mean(n), np.median(n), np.std(n), functools.reduce(lambda x, y: x + y, n), q1, q3)
    return "\t".join(["%i" % len(n)] + ["%6.4f" % x for x in fields])


def summaries(matrix):
    """summary(row) for every row of a [rows, values] matrix, in one pass (the rows of 10 000 samples)"""
    m = np.sort(np.asarray(matrix), axis=1)
    rows, k = m.shape
    if k == 0:
        return [summary([])] * rows
    f = m.astype(np.float64)
    total = m.sum(axis=1) if m.dtype.kind == "i" else np.add.accumulate(f, axis=1)[:, -1]      # (left to right, as reduce adds)
    cols = (m[:, 0], m[:, -1], f.mean(axis=1), np.median(f, axis=1), f.std(axis=1), total, m[:, k // 4], m[:, k * 3 // 4])
    fmt = "%i" + "\t%6.4f" * 8
    return [fmt % ((k,) + t) for t in zip(*(c.tolist() for c in cols))]


def write_rows(outfile, track, sections, words, workspace_bases):
    """IO.outputMetrics for every section: words[section][key][8] against workspace_bases[key]; ten rows a section, the
    sections in order"""
    words = np.asarray(words, dtype=np.int64)
    attrs = attributes(words, np.asarray(workspace_bases, dtype=np.int64)[None, :])
    text = [summaries(a) for a in attrs]
    for i, section in enumerate(sections):
        outfile.write("".join("%s\t%s\t%s\t%s\n" % (track, section, name, text[k][i]) for k, name in enumerate(ATTRIBUTES)))
    outfile.flush()


def contig_workspace(workspace, contigs):
    """the pieces a contig's samples are measured against, for `contigs` in order: (SEG array, CSR offsets, bases per contig).
    workspace: the run's IntervalDictionary (isochore level)"""
    per = problem.from_isochores(workspace.asArrays())
    lists = [per.get(c, iv.EMPTY) for c in contigs]
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(a) for a in lists], out=off[1:])
    data = np.concatenate(lists) if off[-1] else iv.EMPTY.copy()
    size = np.array([int((a["end"].astype(np.int64) - a["start"]).sum()) for a in lists], dtype=np.int64)
    return data, off, size


def present_contigs(flat):
    """the keys of a sample: contigs with at least one unit computeSample does not skip (gat/__init__.py:536-538) -- the
    problem's contigs, the same for every sample"""
    return list(flat["contig_names"])


def write_sample_metrics(outfile, track, P, flat, workspace, seed, num_samples):
    """the sample_metrics rows of one segment track: samples 0..num_samples-1 of problem P (flat: its description) from the
    unit streams of `seed` -- the samples its counts are made from"""
    contigs = present_contigs(flat)
    ws, ws_off, size = contig_workspace(workspace, contigs)
    words = P.sample_metrics(seed, 0, num_samples, ws, ws_off)
    write_rows(outfile, track, [str(i) for i in range(num_samples)], words, size)


def write_empty_sample_metrics(outfile, track, num_samples):
    """... of a track without a unit to sample: every sample is an empty dictionary"""
    write_rows(outfile, track, [str(i) for i in range(num_samples)], np.zeros((num_samples, 0, len(WORDS)), dtype=np.int64), [])


def write_segment_metrics(outfile, segments, workspace, ctx=None):
    """run()'s segment_metrics block (gat/__init__.py:913-925): the header, then per segment track the input segments of
    every isochore-level key against the workspace of that key (empty where the workspace lacks it)"""
    from . import _lib
    from .engine import get_context
    outfile.write(HEADER)
    wa = workspace.asArrays()
    for track in segments.tracks:
        sa = segments[track].asArrays()
        keys = list(sa.keys())
        if not keys:
            write_rows(outfile, track, ["segments"], np.zeros((1, 0, len(WORDS)), dtype=np.int64), [])
            continue
        lists = [sa[k] for k in keys]
        pieces = [wa.get(k, iv.EMPTY) for k in keys]
        list_off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
        ws_off = np.concatenate([[0], np.cumsum([len(a) for a in pieces])]).astype(np.int64)
        cat = (lambda xs, off: np.concatenate(xs) if off[-1] else iv.EMPTY.copy())
        ctx = ctx or get_context()
        words = _lib.list_metrics(ctx, cat(lists, list_off), list_off, 1, cat(pieces, ws_off), ws_off, len(keys))
        size = [int((a["end"].astype(np.int64) - a["start"]).sum()) for a in pieces]
        write_rows(outfile, track, ["segments"], words, size)
