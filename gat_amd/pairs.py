"""gat-pairs: are the segments found where annotation A AND annotation B are both present more often than chance would have it?

gat-run tests every annotation on its own.  With many tracks the next question is about combinations, and the table gat-run
writes cannot answer it: a segment that hits both A and B is not two independent events -- the tracks overlap each other,
cluster and share isochores -- and the expected value is not the product of the marginal ones.  Only the null model knows it.
Here every pair of annotation tracks (i, j), i <= j, gets gat-run's test of the count

    c = the segments that share a base with an interval of track i and with an interval of track j

against the same count of every sampled segment list (i == j: the segments that hit the track, CounterSegmentOverlap).  The
(samples x pairs) matrix is never formed: the null is reduced on the device where the sampler leaves its lists (k_pairs
behind every batch, gat_sample_pair_enrichment) to five integers per pair -- n_pos, sum, sumsq, n_less, n_eq;
include/gat_mi355.h has the definition -- and the row's statistics are made from those with enrichment.bin_statistics.  The observed
values come from gat_list_pair_hits on the input segments.  Segments and annotations are both taken to contig level
(problem.from_isochores).  A row is written for every pair i < j that holds an observed or a sampled hit (--include-single:
the pairs (i, i) too); q-values are over the rows written, per segment track.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import math

import numpy as np

from . import enrichment
from . import problem
from .engine import AnnotatorResult, get_context

TOOL = "gat-pairs"
WORDS, QVALUE_METHODS, bin_statistics = enrichment.WORDS, enrichment.QVALUE_METHODS, enrichment.bin_statistics
flatten, make_sampler, build_inputs = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs
MAX_TRACKS = 2048                         # annotation tracks of one call (GAT_PAIR_MAX_TRACKS): 2 098 176 pairs
HEADER = ("track", "annotation_a", "annotation_b", "observed", "expected", "stddev", "fold", "l2fold", "pvalue", "qvalue",
          "samples_with_hit", "observed_a", "observed_b")
ORDERS = ("track", "annotation", "fold", "pvalue", "qvalue", "observed")


def pair_index(n_tracks):
    """k[i, j] = k[j, i] = the index of the pair of tracks i and j among the n_tracks * (n_tracks + 1) / 2 pairs, ordered
    (0,0), (0,1), .., (0,T-1), (1,1), ..: i * T - i * (i - 1) / 2 + (j - i) for i <= j.  int64 [n_tracks, n_tracks]."""
    T = int(n_tracks)
    t = np.arange(T, dtype=np.int64)
    i, j = np.minimum.outer(t, t), np.maximum.outer(t, t)
    return i * T - i * (i - 1) // 2 + (j - i)


class PairResult(object):
    """a row of the table: one (segment track, annotation a, annotation b)"""
    format_observed = AnnotatorResult.format_observed
    format_expected = AnnotatorResult.format_expected
    format_fold = AnnotatorResult.format_fold
    format_pvalue = AnnotatorResult.format_pvalue
    headers = list(HEADER)

    def __init__(self, track, annotation_a, annotation_b, observed, words, num_samples, observed_a, observed_b, pseudo_count=1.0,
                 position=0):
        self.track, self.annotation_a, self.annotation_b = track, annotation_a, annotation_b
        self.observed, self.nsamples = int(observed), int(num_samples)
        self.observed_a, self.observed_b = int(observed_a), int(observed_b)
        self.words = tuple(int(w) for w in words)
        self.samples_with_hit = self.words[0]
        self.expected, self.stddev, self.fold, self.pvalue = bin_statistics(observed, words, num_samples, pseudo_count)
        self.qvalue = 1.0
        self.position = position              # (the pair's index: annotation a, then annotation b, in the tracks' order)

    def __str__(self):
        logfold = self.format_fold % math.log(self.fold, 2) if self.fold > 0 else "-inf"
        return "\t".join((self.track, self.annotation_a, self.annotation_b, self.format_observed % self.observed,
                          self.format_expected % self.expected, self.format_expected % self.stddev, self.format_fold % self.fold,
                          logfold, self.format_pvalue % self.pvalue, self.format_pvalue % self.qvalue,
                          "%i" % self.samples_with_hit, self.format_observed % self.observed_a,
                          self.format_observed % self.observed_b))


def rows(track, annotations, observed, words, num_samples, pseudo_count=1.0, include_single=False):
    """the rows of one segment track: observed [P], words [P][5], annotations the names in the tracks' order.  One row per
    pair i < j (include_single: i <= j) with observed > 0 or sum > 0, in the pairs' order."""
    observed, words = np.asarray(observed, dtype=np.int64), np.asarray(words, dtype=np.int64)
    k = pair_index(len(annotations))
    out = []
    for i, a in enumerate(annotations):
        for j in range(i if include_single else i + 1, len(annotations)):
            p = int(k[i, j])
            if observed[p] > 0 or words[p, 1] > 0:
                out.append(PairResult(track, a, annotations[j], observed[p], words[p], num_samples, observed[k[i, i]], observed[k[j, j]],
                                      pseudo_count, position=p))
    return out


def set_qvalues(results, method="BH"):
    """q-values over the rows written, per segment track"""
    enrichment.set_qvalues(results, method, TOOL)


def check_options(options):
    """what gat-pairs does not do, refused before anything is read"""
    enrichment.check_options(options, TOOL)


def track_pairs(track, segs, annotations, workspace, sampler, num_samples, random_seed=None, pseudo_count=1.0, include_single=False,
                ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `annotations` the IntervalCollection.  Returns (rows, the problem's unit count)."""
    from . import _lib
    num_samples, seed, flat, _, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names = list(annotations.tracks)
    if not contigs or not names:
        return [], flat["n_units"]
    if len(names) > MAX_TRACKS:
        raise ValueError("gat-pairs: %d annotation tracks are more than %d (%d pairs)" % (len(names), MAX_TRACKS, MAX_TRACKS * (MAX_TRACKS + 1) // 2))
    annos, anno_off = enrichment.contig_lists([problem.from_isochores(annotations[t].asArrays()) for t in names], contigs)
    ctx = ctx or get_context()
    observed = ctx.list_pair_hits(lists, list_off, 1, annos, anno_off, len(names), len(contigs))[0]
    P = _lib.Problem(ctx, flat)
    try:
        words = P.sample_pair_enrichment(seed, 0, num_samples, annos, anno_off, len(names), observed)
    finally:
        P.close()
    return rows(track, names, observed, words, num_samples, pseudo_count, include_single), flat["n_units"]


def run(segments, annotations, workspace, sampler, num_samples, random_seed=None, pseudo_count=1.0, qvalue_method="BH",
        include_single=False, ctx=None):
    """every segment track against every pair of annotation tracks: the PairResults track by track.  random_seed: base of
    the per-unit streams (None: drawn from numpy's global RandomState); every track takes the next num_samples * n_units
    streams, as gat.run hands them out."""
    return enrichment.run_tracks(segments, lambda track, segs, seed: track_pairs(
        track, segs, annotations, workspace, sampler, num_samples, seed, pseudo_count, include_single, ctx), num_samples, random_seed, qvalue_method, TOOL)


def write_results(outfile, results, order="track"):
    """the table, rows ordered by --order (ties in the pairs' order)"""
    enrichment.write_results(outfile, results, HEADER, {"track": lambda x: (x.track, x.position), "annotation": lambda x: (x.position, x.track)}, order)
