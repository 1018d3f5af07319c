"""gat-local: where along the genome do the segments overlap an annotation more (or less) than chance would have it?

gat-run gives one number per annotation -- the overlap over the whole workspace and its p-value.  This is the question
behind a significant row: one locus, one chromosome arm, or everywhere?  The genome is cut into bins of --bin-size bases
(bin b of a contig is [b * bin_size, (b + 1) * bin_size); a contig has ceil(largest workspace end / bin_size) bins, as in
gat-coverage) and every (annotation, bin) gets the test gat-run makes for the annotation: the observed value

    v = | segments n annotation n bin |        bases

against the same value of every sampled segment list.  The (samples x annotations x bins) matrix is never formed: the null is
reduced on the device where the sampler leaves its lists (k_local behind every batch, gat_sample_bin_enrichment) to five
integers per (annotation, bin) -- n_pos, sum, sumsq, n_less, n_eq; include/gat_mi355.h has the definition -- and the row's
statistics are made from those: expected = sum / S, stddev from sum and sumsq, the empirical p-value from n_less and n_eq with
the arithmetic of AnnotatorResult._two_sided (engine.twoSidedPValueFromCounts).  The observed values come from
gat_list_bin_overlaps on the input segments.  Segments and annotations are both taken to contig level
(problem.from_isochores).  A row is written for every (annotation, bin) that holds an observed or a sampled base; q-values are
over the rows written, per segment track.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import math

import numpy as np

from . import enrichment
from . import problem
from .engine import AnnotatorResult, get_context

TOOL = "gat-local"
WORDS, QVALUE_METHODS, bin_statistics = enrichment.WORDS, enrichment.QVALUE_METHODS, enrichment.bin_statistics
flatten, make_sampler, build_inputs = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs
BIN_SIZE = 100000
MAX_CELLS = 2 ** 27                       # tracks x bins of one call: five int64 words each on the device and on the host
HEADER = ("track", "annotation", "contig", "start", "end", "observed", "expected", "stddev", "fold", "l2fold", "pvalue", "qvalue",
          "samples_with_overlap")
ORDERS = ("track", "annotation", "fold", "pvalue", "qvalue", "observed")


class LocalResult(object):
    """a row of the table: one (segment track, annotation, bin)"""
    format_observed = AnnotatorResult.format_observed
    format_expected = AnnotatorResult.format_expected
    format_fold = AnnotatorResult.format_fold
    format_pvalue = AnnotatorResult.format_pvalue
    headers = list(HEADER)

    def __init__(self, track, annotation, contig, start, end, observed, words, num_samples, pseudo_count=1.0, position=0):
        self.track, self.annotation, self.contig, self.start, self.end = track, annotation, contig, int(start), int(end)
        self.observed, self.nsamples = int(observed), int(num_samples)
        self.words = tuple(int(w) for w in words)
        self.samples_with_overlap = self.words[0]
        self.expected, self.stddev, self.fold, self.pvalue = bin_statistics(observed, words, num_samples, pseudo_count)
        self.qvalue = 1.0
        self.position = position              # (rank of the bin in the genome: contig in the problem's order, then start)

    def __str__(self):
        logfold = self.format_fold % math.log(self.fold, 2) if self.fold > 0 else "-inf"
        return "\t".join((self.track, self.annotation, self.contig, "%i" % self.start, "%i" % self.end,
                          self.format_observed % self.observed, self.format_expected % self.expected,
                          self.format_expected % self.stddev, self.format_fold % self.fold, logfold,
                          self.format_pvalue % self.pvalue, self.format_pvalue % self.qvalue, "%i" % self.samples_with_overlap))


def rows(track, annotations, contigs, bin_off, bin_size, observed, words, num_samples, pseudo_count=1.0):
    """the rows of one segment track: observed [n_tracks][total_bins], words [n_tracks][total_bins][5], annotations and
    contigs the names in the arrays' order, contig c's bins at [bin_off[c], bin_off[c + 1]).  One row per (annotation, bin)
    with observed > 0 or sum > 0, annotation by annotation along the genome."""
    observed, words = np.asarray(observed, dtype=np.int64), np.asarray(words, dtype=np.int64)
    bin_off = np.asarray(bin_off, dtype=np.int64)
    out = []
    for t, a in enumerate(annotations):
        keep = np.flatnonzero((observed[t] > 0) | (words[t, :, 1] > 0))
        which = np.searchsorted(bin_off, keep, side="right") - 1
        for k, c in zip(keep.tolist(), which.tolist()):
            b = k - int(bin_off[c])
            out.append(LocalResult(track, a, contigs[c], b * bin_size, (b + 1) * bin_size, observed[t, k], words[t, k], num_samples,
                                   pseudo_count, position=k))
    return out


def set_qvalues(results, method="BH"):
    """q-values over the rows written, per segment track"""
    enrichment.set_qvalues(results, method, TOOL)


def check_options(options):
    """what gat-local does not do, refused before anything is read"""
    enrichment.check_options(options, TOOL)


def bins_per_contig(contig_ws, contigs, bin_size):
    """ceil(largest workspace end / bin_size) per contig, as gat-coverage has it"""
    n_bins = []
    for c in contigs:
        w = contig_ws.get(c)
        top = int(w["end"].max()) if w is not None and len(w) else 0
        n_bins.append((top + bin_size - 1) // bin_size)
    return n_bins


def track_local(track, segs, annotations, workspace, sampler, num_samples, bin_size=BIN_SIZE, random_seed=None, pseudo_count=1.0,
                ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `annotations` the IntervalCollection.  Returns (rows, the problem's unit count)."""
    from . import _lib
    bin_size = int(bin_size)
    if not 1 <= bin_size <= 2 ** 31:
        raise ValueError("bin_size %d outside [1, 2^31]" % bin_size)
    num_samples, seed, flat, wa, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names = list(annotations.tracks)
    if not contigs or not names:
        return [], flat["n_units"]
    n_bins = bins_per_contig(problem.from_isochores(wa), contigs, bin_size)
    if len(names) * sum(n_bins) > MAX_CELLS:
        raise ValueError("gat-local: %d annotations x %d bins of %d bases are more than 2^27 (annotation, bin) pairs: choose a larger "
                         "--bin-size" % (len(names), sum(n_bins), bin_size))
    annos, anno_off = enrichment.contig_lists([problem.from_isochores(annotations[t].asArrays()) for t in names], contigs)
    ctx = ctx or get_context()
    observed, bin_off = ctx.list_bin_overlaps(lists, list_off, 1, annos, anno_off, len(names), len(contigs), bin_size, n_bins)
    P = _lib.Problem(ctx, flat)
    try:
        words, _ = P.sample_bin_enrichment(seed, 0, num_samples, annos, anno_off, len(names), bin_size, n_bins, observed[0])
    finally:
        P.close()
    return rows(track, names, contigs, bin_off, bin_size, observed[0], words, num_samples, pseudo_count), flat["n_units"]


def run(segments, annotations, workspace, sampler, num_samples, bin_size=BIN_SIZE, random_seed=None, pseudo_count=1.0,
        qvalue_method="BH", ctx=None):
    """every segment track against every annotation track, bin by bin: the LocalResults track by track.  random_seed: base of
    the per-unit streams (None: drawn from numpy's global RandomState); every track takes the next num_samples * n_units
    streams, as gat.run hands them out."""
    return enrichment.run_tracks(segments, lambda track, segs, seed: track_local(
        track, segs, annotations, workspace, sampler, num_samples, bin_size, seed, pseudo_count, ctx), num_samples, random_seed, qvalue_method, TOOL)


def write_results(outfile, results, order="track"):
    """the table, rows ordered by --order (ties along the genome)"""
    enrichment.write_results(outfile, results, HEADER, {"track": lambda x: (x.track, x.annotation, x.position),
                                                        "annotation": lambda x: (x.annotation, x.track, x.position)}, order)
