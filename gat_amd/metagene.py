"""gat-metagene: how are the segments distributed along a class of features -- genes, enhancers, CpG islands -- once every
feature is stretched to the same length, and is that shaped differently from chance?

gat-profile bins absolute offsets from one point: genes of 2 kb and of 200 kb do not align beyond the anchor.  Here every
feature track gets the metagene (the scaled-region profile) of the segments: every feature is cut into body_bins bins of equal
share, 5' to 3' by its strand, with flank_bins bins of flank_bin_size bases upstream and downstream -- B = 2 * flank_bins +
body_bins bins.  For a plus feature [fs, fe) and F = flank_bins * flank_bin_size, base x of the window [fs - F, fe + F) lies

    upstream    x < fs          in bin floor((x - (fs - F)) / flank_bin_size)
    body        fs <= x < fe    in bin flank_bins + floor((x - fs) * body_bins / (fe - fs))
    downstream  x >= fe         in bin flank_bins + body_bins + floor((x - fe) / flank_bin_size)

and a minus feature is the mirror, x -> fs + fe - 1 - x.  The value of a (feature track, bin) is

    v = the bases of the segments (--profile-of=bases) or their midpoints (midpoints) in the bin, summed over the features

a base counting once per feature whose window holds it -- overlapping and nested genes each get it, as an aggregate plot does.
Every (feature track, bin) gets the test gat-run makes for an annotation: the observed v against the same value of every
sampled segment list.  Only the sampled lists calibrate that bins of long genes hold more bases, that genes cluster in
GC-rich isochores and that overlapping genes count a base twice.  The (samples x tracks x bins) matrix is never formed: the null
is reduced on the device where the sampler leaves its lists (k_metagene behind every batch, gat_sample_metagene_enrichment) to
five integers per cell -- n_pos, sum, sumsq, n_less, n_eq; include/gat_mi355.h has the definition -- and the row's statistics
are made from those (enrichment.bin_statistics).  The observed values come from gat_list_metagene on the input segments, taken
to contig level (problem.from_isochores).  A metagene is plotted whole: every bin of every feature track with at least one
feature on the problem's contigs is written, zeros included; q-values are over the rows written, per segment track.

The features are read here (read_features): io.readFromBed drops the strand column, and normalizing would unite overlapping
genes.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import collections
import math
import os

import numpy as np

from . import enrichment
from .engine import AnnotatorResult, get_context
from .profile import _stranded_bed_lines

TOOL = "gat-metagene"
WORDS, QVALUE_METHODS, bin_statistics = enrichment.WORDS, enrichment.QVALUE_METHODS, enrichment.bin_statistics
flatten, make_sampler, build_inputs = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs
BODY_BINS, FLANK_BINS, FLANK_BIN_SIZE = 50, 20, 100
MAX_BINS = 1024                           # GAT_METAGENE_MAX_BINS
PROFILES_OF = ("bases", "midpoints")      # GAT_METAGENE_BASES, GAT_METAGENE_MIDPOINTS
REGIONS = ("upstream", "body", "downstream")
HEADER = ("track", "annotation", "bin", "region", "rel_start", "rel_end", "observed", "expected", "stddev", "fold", "l2fold", "pvalue",
          "qvalue", "samples_with_overlap", "features")
ORDERS = ("track", "annotation", "fold", "pvalue", "qvalue", "observed")
_NONE = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8))


def read_features(filenames, min_length=1, ignore_strand=False, label=None, log=None):
    """the features of BED files: OrderedDict track -> OrderedDict contig -> (starts uint32, ends uint32, minus uint8), tracks in
    the order of their first line and a track's contigs in the order of theirs, as io.readFromBed has them; a (track, contig)'s
    features ascending by (start, end, minus), a repeated (start, end, strand) once -- alternative transcripts with one span
    are one feature.  Features overlap and nest; nothing is merged or cut.  Features shorter than min_length
    (--min-feature-length; the tool's default is --body-bins: a shorter feature leaves body bins without a base) are dropped
    and counted: log(line) is told how many.  Track names follow io.readFromBed: the `track name=` line, else column 4, else
    the file's base name; with `label` (--annotations-label) everything is one track, 'merged', as the annotation collection
    has it.  Column 6 `-` is the minus strand; anything else, or fewer than six columns, is plus; ignore_strand: every feature
    is plus."""
    if isinstance(filenames, str):
        filenames = [filenames]
    seen = collections.OrderedDict()        # track -> contig -> set of (start, end, minus)
    short = 0
    for filename in filenames:
        for name, contig, start, end, strand in _stranded_bed_lines(filename, os.path.basename(filename), label is not None):
            if not 0 <= start < end < 2 ** 32:
                raise ValueError("%s: feature [%d, %d) on %s in %s is empty or outside [0, 2^32 - 1]" % (TOOL, start, end, contig, filename))
            per = seen.setdefault(name, collections.OrderedDict()).setdefault(contig, set())
            if end - start < int(min_length):
                short += 1
                continue
            per.add((start, end, int(strand == "-" and not ignore_strand)))
    if short and log:
        log("%s: %d features shorter than %d bases dropped (--min-feature-length)" % (TOOL, short, int(min_length)))
    features = collections.OrderedDict()
    for name, per in seen.items():
        features[name] = collections.OrderedDict()
        for contig, keys in per.items():
            keys = np.array(sorted(keys), dtype=np.int64).reshape(-1, 3)
            features[name][contig] = (keys[:, 0].astype(np.uint32), keys[:, 1].astype(np.uint32), keys[:, 2].astype(np.uint8))
    return features


def feature_arrays(features, contigs):
    """what the library takes of the feature tracks with at least one feature on `contigs`: (names, starts, ends, minus,
    offsets, features per track) -- track t of contig c at offsets[t * len(contigs) + c]; features on other contigs are dropped"""
    names, cols, counts, totals = [], ([], [], []), [], []
    for name, per in features.items():
        total = sum(len(per[c][0]) for c in contigs if c in per)
        if total == 0:
            continue
        names.append(name)
        totals.append(total)
        for c in contigs:
            triple = per.get(c, _NONE)
            for col, a in zip(cols, triple):
                col.append(a)
            counts.append(len(triple[0]))
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    if counts:
        np.cumsum(counts, out=off[1:])
    fs, fe, minus = (np.concatenate(col) if col else none for col, none in zip(cols, _NONE))
    return names, fs, fe, minus, off, totals


def bin_region(b, body_bins, flank_bins, flank_bin_size):
    """(region, rel_start, rel_end) of bin b as the table prints them: a flank bin covers the bases [rel_start, rel_end) from
    the feature's 5' end (upstream: negative) or from its 3' end (downstream: from 0); a body bin the fractions
    [k / body_bins, (k + 1) / body_bins) of the feature, as text with six decimals"""
    b, Bb, Bf, w = int(b), int(body_bins), int(flank_bins), int(flank_bin_size)
    if b < Bf:
        return REGIONS[0], "%i" % ((b - Bf) * w), "%i" % ((b + 1 - Bf) * w)
    if b < Bf + Bb:
        return REGIONS[1], "%.6f" % ((b - Bf) / Bb), "%.6f" % ((b - Bf + 1) / Bb)
    return REGIONS[2], "%i" % ((b - Bf - Bb) * w), "%i" % ((b + 1 - Bf - Bb) * w)


class MetageneResult(object):
    """a row of the table: one (segment track, feature track, bin)"""
    format_observed = AnnotatorResult.format_observed
    format_expected = AnnotatorResult.format_expected
    format_fold = AnnotatorResult.format_fold
    format_pvalue = AnnotatorResult.format_pvalue
    headers = list(HEADER)

    def __init__(self, track, annotation, bin, region, rel_start, rel_end, observed, words, num_samples, features, pseudo_count=1.0):
        self.track, self.annotation, self.bin = track, annotation, int(bin)
        self.region, self.rel_start, self.rel_end, self.features = region, rel_start, rel_end, int(features)
        self.observed, self.nsamples = int(observed), int(num_samples)
        self.words = tuple(int(w) for w in words)
        self.samples_with_overlap = self.words[0]
        self.expected, self.stddev, self.fold, self.pvalue = bin_statistics(observed, words, num_samples, pseudo_count)
        self.qvalue = 1.0

    def __str__(self):
        logfold = self.format_fold % math.log(self.fold, 2) if self.fold > 0 else "-inf"
        return "\t".join((self.track, self.annotation, "%i" % self.bin, self.region, self.rel_start, self.rel_end,
                          self.format_observed % self.observed, self.format_expected % self.expected,
                          self.format_expected % self.stddev, self.format_fold % self.fold, logfold,
                          self.format_pvalue % self.pvalue, self.format_pvalue % self.qvalue, "%i" % self.samples_with_overlap,
                          "%i" % self.features))


def rows(track, annotations, n_features, body_bins, flank_bins, flank_bin_size, observed, words, num_samples, pseudo_count=1.0):
    """the rows of one segment track: observed [n_tracks][B], words [n_tracks][B][5], annotations the feature tracks' names and
    n_features their features, in the arrays' order.  Every bin of every track is a row, zeros included: a metagene is plotted
    whole."""
    observed, words = np.asarray(observed, dtype=np.int64), np.asarray(words, dtype=np.int64)
    out = []
    for t, a in enumerate(annotations):
        for b in range(2 * int(flank_bins) + int(body_bins)):
            region, rel_start, rel_end = bin_region(b, body_bins, flank_bins, flank_bin_size)
            out.append(MetageneResult(track, a, b, region, rel_start, rel_end, observed[t, b], words[t, b], num_samples, n_features[t],
                                      pseudo_count))
    return out


def set_qvalues(results, method="BH"):
    """q-values over the rows written, per segment track"""
    enrichment.set_qvalues(results, method, TOOL)


def check_geometry(body_bins, flank_bins, flank_bin_size, profile_of="bases"):
    """body_bins >= 1, flank_bins >= 0, 2 * flank_bins + body_bins <= 1024, flank_bin_size in [1, 2^31], flank_bins *
    flank_bin_size <= 2^31, as the library asks"""
    body_bins, flank_bins, flank_bin_size = int(body_bins), int(flank_bins), int(flank_bin_size)
    if body_bins < 1:
        raise ValueError("%s: --body-bins=%d is less than 1" % (TOOL, body_bins))
    if flank_bins < 0:
        raise ValueError("%s: --flank-bins=%d is negative" % (TOOL, flank_bins))
    if 2 * flank_bins + body_bins > MAX_BINS:
        raise ValueError("%s: 2 x --flank-bins + --body-bins = %d bins is more than %d" % (TOOL, 2 * flank_bins + body_bins, MAX_BINS))
    if not 1 <= flank_bin_size <= 2 ** 31:
        raise ValueError("%s: --flank-bin-size=%d is outside [1, 2^31]" % (TOOL, flank_bin_size))
    if flank_bins * flank_bin_size > 2 ** 31:
        raise ValueError("%s: --flank-bins x --flank-bin-size = %d bases to either side is more than 2^31" % (TOOL, flank_bins * flank_bin_size))
    if profile_of not in PROFILES_OF:
        raise ValueError("%s: --profile-of=%s is not one of %s" % (TOOL, profile_of, ", ".join(PROFILES_OF)))
    return body_bins, flank_bins, flank_bin_size, PROFILES_OF.index(profile_of)


def min_feature_length(options):
    """--min-feature-length, which defaults to --body-bins"""
    given = getattr(options, "min_feature_length", None)
    return int(getattr(options, "body_bins", BODY_BINS)) if given is None else int(given)


def check_options(options):
    """what gat-metagene does not do, refused before anything is read"""
    enrichment.check_options(options, TOOL, "a feature is scaled over its whole span")
    check_geometry(getattr(options, "body_bins", BODY_BINS), getattr(options, "flank_bins", FLANK_BINS),
                   getattr(options, "flank_bin_size", FLANK_BIN_SIZE), getattr(options, "profile_of", "bases"))
    if min_feature_length(options) < 1:
        raise ValueError("%s: --min-feature-length=%d is less than 1" % (TOOL, min_feature_length(options)))


def track_metagene(track, segs, features, workspace, sampler, num_samples, body_bins=BODY_BINS, flank_bins=FLANK_BINS,
                   flank_bin_size=FLANK_BIN_SIZE, profile_of="bases", random_seed=None, pseudo_count=1.0, ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `features` what read_features returns.  Returns (rows, the problem's unit count)."""
    from . import _lib
    body_bins, flank_bins, flank_bin_size, mode = check_geometry(body_bins, flank_bins, flank_bin_size, profile_of)
    num_samples, seed, flat, wa, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names, fs, fe, minus, off, n_features = feature_arrays(features, contigs)
    if not contigs or not names:
        return [], flat["n_units"]
    ctx = ctx or get_context()
    geometry = (body_bins, flank_bins, flank_bin_size, mode)
    observed = ctx.list_metagene(lists, list_off, 1, fs, fe, minus, off, len(names), len(contigs), *geometry)
    P = _lib.Problem(ctx, flat)
    try:
        words = P.sample_metagene_enrichment(seed, 0, num_samples, fs, fe, minus, off, len(names), *geometry, observed[0])
    finally:
        P.close()
    return rows(track, names, n_features, body_bins, flank_bins, flank_bin_size, observed[0], words, num_samples, pseudo_count), flat["n_units"]


def run(segments, features, workspace, sampler, num_samples, body_bins=BODY_BINS, flank_bins=FLANK_BINS, flank_bin_size=FLANK_BIN_SIZE,
        profile_of="bases", random_seed=None, pseudo_count=1.0, qvalue_method="BH", ctx=None):
    """every segment track along every feature track: the MetageneResults track by track.  random_seed: base of the per-unit
    streams (None: drawn from numpy's global RandomState); every track takes the next num_samples * n_units streams, as
    gat.run hands them out."""
    return enrichment.run_tracks(segments, lambda track, segs, seed: track_metagene(
        track, segs, features, workspace, sampler, num_samples, body_bins, flank_bins, flank_bin_size, profile_of, seed, pseudo_count, ctx),
        num_samples, random_seed, qvalue_method, TOOL)


def write_results(outfile, results, order="track"):
    """the table, rows ordered by --order (ties by bin)"""
    enrichment.write_results(outfile, results, HEADER, {"track": lambda x: (x.track, x.annotation, x.bin),
                                                        "annotation": lambda x: (x.annotation, x.track, x.bin)}, order)
