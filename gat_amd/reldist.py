"""gat-reldist: do the segments sit closer to -- or further from -- the features of an annotation than chance puts them,
whatever the density of the features?

The relative distance test (bedtools reldist, GenometriCorr).  Every interval of an annotation is a reference point
(--annotation-point: its midpoint, start or last base).  A segment stands for its midpoint m; where two points of the annotation
flank it, p <= m < p', it is inside, and its relative distance is min(m - p, p' - m) / (p' - p), in [0, 0.5].  If segments and
features ignore each other that fraction is spread evenly; mass near 0 is attraction, mass near 0.5 avoidance.  It works where
overlap fails -- on features that are points, or sparse -- and where gat-distance cannot help: an absolute distance confounds
association with feature density, a relative one does not.  An (annotation, value) is

    bin b of --bins     the inside segments with floor(2 * d * bins / gap) == b (0.5 itself in the last bin)
    area                the area between the ECDF of the segments over the bins and the uniform one, 0 .. 1
    inside, outside     the segments with and without two flanking points

and each gets the test gat-run makes for an annotation: the observed value against the same value of every sampled segment
list.  bedtools prints only the histogram and GenometriCorr tests against a uniform null, which is wrong inside a fragmented
workspace, with isochores, or with clustered segments; here the null is the sampler's.  The (samples x annotations x values)
matrix is never formed: the null is reduced on the device where the sampler leaves its lists (k_reldist behind every batch,
gat_sample_reldist_enrichment) to five integers per cell -- n_pos, sum, sumsq, n_less, n_eq; include/gat_mi355.h has the
definition -- and the row's statistics are made from those (enrichment.bin_statistics).  The observed values come from
gat_list_reldist on the input segments, taken to contig level (problem.from_isochores).  Every bin row of every annotation
with two points on some contig of the problem is written, zeros included; q-values are per segment track, over the bin rows
and separately over the area rows.

The annotations are the normalized interval tracks gat-distance reads, taken to contig level: disjoint, non-empty intervals,
whose midpoints, starts and last bases are each strictly ascending (points_of asserts it).

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import math

import numpy as np

from . import enrichment
from . import intervals as iv
from . import problem
from .engine import AnnotatorResult, get_context

TOOL = "gat-reldist"
WORDS, QVALUE_METHODS, bin_statistics = enrichment.WORDS, enrichment.QVALUE_METHODS, enrichment.bin_statistics
flatten, make_sampler, build_inputs = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs
BINS = 50
MAX_BINS = 1024                           # GAT_RELDIST_MAX_BINS
AREA_SCALE = 10 ** 6                      # GAT_RELDIST_AREA_SCALE
SUMMARIES = ("area", "inside", "outside") # the values behind the bins, in the library's order (GAT_RELDIST_EXTRA)
ANNOTATION_POINTS = ("midpoint", "start", "end")
HEADER = ("track", "annotation", "bin", "reldist_start", "reldist_end", "observed", "expected", "stddev", "fold", "l2fold", "pvalue",
          "qvalue", "samples_with_hit", "points")
ORDERS = ("track", "annotation", "fold", "pvalue", "qvalue", "observed")


def points_of(intervals, annotation_point="midpoint"):
    """the reference points (uint32, strictly ascending) of a normalized interval list (SEG array: sorted, disjoint, none
    empty): midpoint -- start + (end - start) // 2; start; end -- the last base, end - 1.  Disjoint non-empty intervals have
    s_i < e_i <= s_{i+1}, so s_i < s_{i+1}, e_i - 1 < e_{i+1} - 1 and m_i < e_i <= s_{i+1} <= m_{i+1}: all three ascend strictly."""
    if annotation_point not in ANNOTATION_POINTS:
        raise ValueError("%s: --annotation-point=%s is not one of %s" % (TOOL, annotation_point, ", ".join(ANNOTATION_POINTS)))
    start, end = intervals["start"].astype(np.int64), intervals["end"].astype(np.int64)
    assert np.all(end > start) and np.all(start[1:] >= end[:-1]), "%s: an annotation track is not normalized" % TOOL
    pos = start + (end - start) // 2 if annotation_point == "midpoint" else start if annotation_point == "start" else end - 1
    assert np.all(pos[1:] > pos[:-1])
    return pos.astype(np.uint32)


def point_arrays(annotations, contigs, annotation_point="midpoint"):
    """what the library takes of the annotation tracks with two points on some contig of `contigs`: (names, positions, offsets,
    points per track) -- track t of contig c at offsets[t * len(contigs) + c]; `annotations`: the IntervalCollection, at
    isochore level or not; intervals on other contigs are dropped"""
    names, pos, counts, totals = [], [], [], []
    for name in annotations.tracks:
        per = problem.from_isochores(annotations[name].asArrays())
        mine = [points_of(per[c], annotation_point) if c in per else np.zeros(0, dtype=np.uint32) for c in contigs]
        if not any(len(p) >= 2 for p in mine):
            continue
        names.append(name)
        totals.append(sum(len(p) for p in mine))
        pos.extend(mine)
        counts.extend(len(p) for p in mine)
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    if counts:
        np.cumsum(counts, out=off[1:])
    return names, np.concatenate(pos) if pos else np.zeros(0, dtype=np.uint32), off, totals


class ReldistResult(object):
    """a row of the table: one (segment track, annotation, value) -- a bin, or one of SUMMARIES.  The statistics are made
    from the library's integers; the area row then prints observed, expected and stddev as fractions of 1 (its fold keeps the
    pseudo count in parts per million)."""
    format_observed = AnnotatorResult.format_observed
    format_expected = AnnotatorResult.format_expected
    format_fold = AnnotatorResult.format_fold
    format_pvalue = AnnotatorResult.format_pvalue
    format_reldist = "%.6g"
    headers = list(HEADER)

    def __init__(self, track, annotation, bin, n_bins, observed, words, num_samples, points, pseudo_count=1.0):
        self.track, self.annotation, self.points, self.n_bins = track, annotation, int(points), int(n_bins)
        self.bin = bin if bin in SUMMARIES else int(bin)
        self.is_bin = bin not in SUMMARIES
        self.position = self.bin if self.is_bin else self.n_bins + SUMMARIES.index(bin)
        self.reldist_start = self.bin / (2.0 * self.n_bins) if self.is_bin else 0.0
        self.reldist_end = (self.bin + 1) / (2.0 * self.n_bins) if self.is_bin else 0.5
        self.nsamples = int(num_samples)
        self.words = tuple(int(w) for w in words)
        self.samples_with_hit = self.words[0]
        self.expected, self.stddev, self.fold, self.pvalue = bin_statistics(observed, words, num_samples, pseudo_count)
        self.observed = int(observed)
        if bin == "area":
            self.observed, self.expected, self.stddev = self.observed / AREA_SCALE, self.expected / AREA_SCALE, self.stddev / AREA_SCALE
        self.qvalue = 1.0

    def __str__(self):
        logfold = self.format_fold % math.log(self.fold, 2) if self.fold > 0 else "-inf"
        observed = "%.6f" % self.observed if self.bin == "area" else self.format_observed % self.observed
        return "\t".join((self.track, self.annotation, "%s" % (self.bin,), self.format_reldist % self.reldist_start,
                          self.format_reldist % self.reldist_end, observed, self.format_expected % self.expected,
                          self.format_expected % self.stddev, self.format_fold % self.fold, logfold,
                          self.format_pvalue % self.pvalue, self.format_pvalue % self.qvalue, "%i" % self.samples_with_hit,
                          "%i" % self.points))


def rows(track, annotations, n_points, n_bins, observed, words, num_samples, pseudo_count=1.0):
    """the rows of one segment track: observed [n_tracks][W], words [n_tracks][W][5] with W = n_bins + 3, annotations the
    point tracks' names and n_points their points, in the arrays' order.  Every bin of every track is a row, zeros included,
    then area, inside and outside."""
    observed, words = np.asarray(observed, dtype=np.int64), np.asarray(words, dtype=np.int64)
    n_bins = int(n_bins)
    assert observed.shape == (len(annotations), n_bins + len(SUMMARIES)) and words.shape == observed.shape + (len(WORDS),)
    out = []
    for t, a in enumerate(annotations):
        for k in range(n_bins + len(SUMMARIES)):
            out.append(ReldistResult(track, a, k if k < n_bins else SUMMARIES[k - n_bins], n_bins, observed[t, k], words[t, k],
                                     num_samples, n_points[t], pseudo_count))
    return out


def set_qvalues(results, method="BH"):
    """q-values per segment track: over the bin rows, and separately over the area rows; inside and outside rows keep 1"""
    enrichment.check_qvalue_method(method, TOOL)
    for x in results:
        x.qvalue = 1.0
    enrichment.set_qvalues([x for x in results if x.is_bin], method, TOOL)
    enrichment.set_qvalues([x for x in results if x.bin == "area"], method, TOOL)


def check_bins(n_bins):
    """--bins in [1, 1024], as the library asks"""
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("%s: --bins=%d is outside [1, %d]" % (TOOL, n_bins, MAX_BINS))
    return n_bins


def check_options(options):
    """what gat-reldist does not do, refused before anything is read"""
    enrichment.check_options(options, TOOL, "the point of an annotation interval is chosen with --annotation-point")
    check_bins(getattr(options, "bins", BINS))
    points_of(iv.EMPTY, getattr(options, "annotation_point", "midpoint"))


def track_reldist(track, segs, annotations, workspace, sampler, num_samples, n_bins=BINS, annotation_point="midpoint",
                  random_seed=None, pseudo_count=1.0, ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `annotations` the IntervalCollection.  Returns (rows, the problem's unit count)."""
    from . import _lib
    n_bins = check_bins(n_bins)
    num_samples, seed, flat, wa, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names, pos, off, n_points = point_arrays(annotations, contigs, annotation_point)
    if not contigs or not names:
        return [], flat["n_units"]
    ctx = ctx or get_context()
    observed = ctx.list_reldist(lists, list_off, 1, pos, off, len(names), len(contigs), n_bins)
    P = _lib.Problem(ctx, flat)
    try:
        words = P.sample_reldist_enrichment(seed, 0, num_samples, pos, off, len(names), n_bins, observed[0])
    finally:
        P.close()
    return rows(track, names, n_points, n_bins, observed[0], words, num_samples, pseudo_count), flat["n_units"]


def run(segments, annotations, workspace, sampler, num_samples, n_bins=BINS, annotation_point="midpoint", random_seed=None,
        pseudo_count=1.0, qvalue_method="BH", ctx=None):
    """every segment track against every annotation: the ReldistResults track by track.  random_seed: base of the per-unit
    streams (None: drawn from numpy's global RandomState); every track takes the next num_samples * n_units streams, as
    gat.run hands them out."""
    check_bins(n_bins)
    points_of(iv.EMPTY, annotation_point)
    results = enrichment.run_tracks(segments, lambda track, segs, seed: track_reldist(
        track, segs, annotations, workspace, sampler, num_samples, n_bins, annotation_point, seed, pseudo_count, ctx),
        num_samples, random_seed, qvalue_method, TOOL)
    set_qvalues(results, qvalue_method)           # (run_tracks made one family of a track's rows)
    return results


def write_results(outfile, results, order="track"):
    """the table, rows ordered by --order (ties: the bins, then area, inside, outside)"""
    enrichment.write_results(outfile, results, HEADER, {"track": lambda x: (x.track, x.annotation, x.position),
                                                        "annotation": lambda x: (x.annotation, x.track, x.position)}, order)
