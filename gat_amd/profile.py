"""gat-profile: how are the segments distributed around a class of points -- transcription start sites, motif centres, exon
ends -- and is that shaped differently from chance?

gat-distance reduces a track to two numbers per sample, without sign, strand or shape; gat-local bins absolute coordinates.
Here every anchor track gets the aggregate profile of the segments around its anchors: 2 * half_bins offset bins of bin_size
bases.  An anchor is a position and a strand; the offset of base x from the anchor (a, sigma) is o = sigma * (x - a), so that
negative offsets are upstream; with R = half_bins * bin_size, x is in the window iff -R <= o < R and bin b covers the offsets
[b * bin_size - R, (b + 1) * bin_size - R).  The value of an (anchor track, bin) is

    v = the bases of the segments (--profile-of=bases) or their midpoints (midpoints) in the bin, summed over the anchors

a base counting once per anchor whose window holds it, as an aggregate plot does.  Every (anchor track, bin) gets the test
gat-run makes for an annotation: the observed v against the same value of every sampled segment list.  The (samples x tracks x
bins) matrix is never formed: the null is reduced on the device where the sampler leaves its lists (k_profile behind every
batch, gat_sample_profile_enrichment) to five integers per cell -- n_pos, sum, sumsq, n_less, n_eq; include/gat_mi355.h has
the definition -- and the row's statistics are made from those (enrichment.bin_statistics).  The observed values come from
gat_list_profile on the input segments, taken to contig level (problem.from_isochores).  A profile is plotted whole: every
bin of every anchor track with at least one anchor on the problem's contigs is written, zeros included; q-values are over the
rows written, per segment track.

The anchors are read here (read_anchors): io.readFromBed drops the strand column, and normalizing would unite overlapping genes.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import collections
import math
import os

import numpy as np

from . import enrichment
from . import io as IO
from .engine import AnnotatorResult, get_context

TOOL = "gat-profile"
WORDS, QVALUE_METHODS, bin_statistics = enrichment.WORDS, enrichment.QVALUE_METHODS, enrichment.bin_statistics
flatten, make_sampler, build_inputs = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs
BIN_SIZE, HALF_BINS = 100, 50
MAX_HALF_BINS = 512                       # GAT_PROFILE_MAX_BINS / 2
ANCHOR_POINTS = ("five-prime", "three-prime", "midpoint")
PROFILES_OF = ("bases", "midpoints")      # GAT_PROFILE_BASES, GAT_PROFILE_MIDPOINTS
HEADER = ("track", "annotation", "bin", "offset_start", "offset_end", "observed", "expected", "stddev", "fold", "l2fold", "pvalue",
          "qvalue", "samples_with_overlap", "anchors")
ORDERS = ("track", "annotation", "fold", "pvalue", "qvalue", "observed")


def anchor_position(start, end, minus, anchor_point="five-prime"):
    """the anchor of the interval [start, end) on the plus (minus False) or minus strand: five-prime -- the first base in the
    direction of the strand, start or max(start, end - 1); three-prime -- its mirror; midpoint -- start + (end - start) // 2"""
    if anchor_point == "midpoint":
        return start + (end - start) // 2
    if anchor_point not in ANCHOR_POINTS:
        raise ValueError("%s: --anchor-point=%s is not one of %s" % (TOOL, anchor_point, ", ".join(ANCHOR_POINTS)))
    return max(start, end - 1) if minus == (anchor_point == "five-prime") else start


def _stranded_bed_lines(filename, default_name, ignore_tracks):
    """io._bed_lines with the sixth column: yields (track name, contig, start, end, strand), the strand "" where the line has
    fewer than six columns"""
    track = None
    with IO.openFile(filename, "r") as infile:
        for line in infile:
            if line.startswith("#") or line.startswith("\n"):
                continue
            if line.startswith("track"):
                track = dict((k, v[1:-1] if v[:1] == '"' else v) for k, v in IO._TRACK_RE.findall(line[:-1]))
                continue
            fields = line.rstrip("\r\n").split("\t")
            if len(fields) < 3:
                raise IOError("malformatted entry in %s: %r" % (filename, line))
            if ignore_tracks:
                name = "merged"
            elif track is not None:
                if "name" not in track:
                    raise KeyError("track without field 'name' in file '%s'" % filename)
                name = track["name"]
            elif len(fields) >= 4 and fields[3]:
                name = fields[3]
            else:
                name = default_name
            yield name, fields[0], int(fields[1]), int(fields[2]), fields[5] if len(fields) >= 6 else ""


def read_anchors(filenames, anchor_point="five-prime", ignore_strand=False, label=None):
    """the anchors of BED files: OrderedDict track -> OrderedDict contig -> (positions uint32, minus uint8), tracks in the order
    of their first line and a track's contigs in the order of theirs, as io.readFromBed has them; a (track, contig)'s anchors
    ascending by position, plus before minus at one position, a repeated (position, strand) once -- alternative transcripts
    share a start site.  Track names follow io.readFromBed: the `track name=` line, else column 4, else the file's base name;
    with `label` (--annotations-label) everything is one track, 'merged', as the annotation collection has it.  Column 6 `-` is
    the minus strand; anything else, or fewer than six columns, is plus; ignore_strand: every anchor is plus."""
    if isinstance(filenames, str):
        filenames = [filenames]
    seen = collections.OrderedDict()        # track -> contig -> set of position * 2 + minus
    for filename in filenames:
        for name, contig, start, end, strand in _stranded_bed_lines(filename, os.path.basename(filename), label is not None):
            minus = strand == "-" and not ignore_strand
            pos = anchor_position(start, end, minus, anchor_point)
            if not 0 <= pos < 2 ** 32:
                raise ValueError("%s: anchor position %d on %s in %s is outside [0, 2^32 - 1]" % (TOOL, pos, contig, filename))
            seen.setdefault(name, collections.OrderedDict()).setdefault(contig, set()).add(pos * 2 + int(minus))
    anchors = collections.OrderedDict()
    for name, per in seen.items():
        anchors[name] = collections.OrderedDict()
        for contig, keys in per.items():
            keys = np.array(sorted(keys), dtype=np.int64)
            anchors[name][contig] = ((keys >> 1).astype(np.uint32), (keys & 1).astype(np.uint8))
    return anchors


def anchor_arrays(anchors, contigs):
    """what the library takes of the anchor tracks with at least one anchor on `contigs`: (names, positions, minus, offsets,
    anchors per track) -- track t of contig c at offsets[t * len(contigs) + c]; anchors on other contigs are dropped"""
    names, pos, minus, counts, totals = [], [], [], [], []
    for name, per in anchors.items():
        mine = [per[c] for c in contigs if c in per]
        if sum(len(p) for p, _ in mine) == 0:
            continue
        names.append(name)
        totals.append(sum(len(p) for p, _ in mine))
        for c in contigs:
            p, m = per.get(c, (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)))
            pos.append(p)
            minus.append(m)
            counts.append(len(p))
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    if counts:
        np.cumsum(counts, out=off[1:])
    return (names, np.concatenate(pos) if pos else np.zeros(0, dtype=np.uint32),
            np.concatenate(minus) if minus else np.zeros(0, dtype=np.uint8), off, totals)


class ProfileResult(object):
    """a row of the table: one (segment track, anchor track, offset bin)"""
    format_observed = AnnotatorResult.format_observed
    format_expected = AnnotatorResult.format_expected
    format_fold = AnnotatorResult.format_fold
    format_pvalue = AnnotatorResult.format_pvalue
    headers = list(HEADER)

    def __init__(self, track, annotation, bin, offset_start, offset_end, observed, words, num_samples, anchors, pseudo_count=1.0):
        self.track, self.annotation, self.bin = track, annotation, int(bin)
        self.offset_start, self.offset_end, self.anchors = int(offset_start), int(offset_end), int(anchors)
        self.observed, self.nsamples = int(observed), int(num_samples)
        self.words = tuple(int(w) for w in words)
        self.samples_with_overlap = self.words[0]
        self.expected, self.stddev, self.fold, self.pvalue = bin_statistics(observed, words, num_samples, pseudo_count)
        self.qvalue = 1.0

    def __str__(self):
        logfold = self.format_fold % math.log(self.fold, 2) if self.fold > 0 else "-inf"
        return "\t".join((self.track, self.annotation, "%i" % self.bin, "%i" % self.offset_start, "%i" % self.offset_end,
                          self.format_observed % self.observed, self.format_expected % self.expected,
                          self.format_expected % self.stddev, self.format_fold % self.fold, logfold,
                          self.format_pvalue % self.pvalue, self.format_pvalue % self.qvalue, "%i" % self.samples_with_overlap,
                          "%i" % self.anchors))


def rows(track, annotations, n_anchors, bin_size, half_bins, observed, words, num_samples, pseudo_count=1.0):
    """the rows of one segment track: observed [n_tracks][B], words [n_tracks][B][5], annotations the anchor tracks' names and
    n_anchors their anchors, in the arrays' order.  Every bin of every track is a row, zeros included: a profile is plotted
    whole."""
    observed, words = np.asarray(observed, dtype=np.int64), np.asarray(words, dtype=np.int64)
    bin_size, reach = int(bin_size), int(half_bins) * int(bin_size)
    out = []
    for t, a in enumerate(annotations):
        for b in range(2 * int(half_bins)):
            out.append(ProfileResult(track, a, b, b * bin_size - reach, (b + 1) * bin_size - reach, observed[t, b], words[t, b],
                                     num_samples, n_anchors[t], pseudo_count))
    return out


def set_qvalues(results, method="BH"):
    """q-values over the rows written, per segment track"""
    enrichment.set_qvalues(results, method, TOOL)


def check_geometry(bin_size, half_bins, profile_of="bases"):
    """bin_size in [1, 2^31], half_bins in [1, 512], half_bins * bin_size <= 2^31, as the library asks"""
    bin_size, half_bins = int(bin_size), int(half_bins)
    if not 1 <= bin_size <= 2 ** 31:
        raise ValueError("%s: --bin-size=%d is outside [1, 2^31]" % (TOOL, bin_size))
    if not 1 <= half_bins <= MAX_HALF_BINS:
        raise ValueError("%s: --half-bins=%d is outside [1, %d]" % (TOOL, half_bins, MAX_HALF_BINS))
    if half_bins * bin_size > 2 ** 31:
        raise ValueError("%s: --half-bins x --bin-size = %d bases to either side is more than 2^31" % (TOOL, half_bins * bin_size))
    if profile_of not in PROFILES_OF:
        raise ValueError("%s: --profile-of=%s is not one of %s" % (TOOL, profile_of, ", ".join(PROFILES_OF)))
    return bin_size, half_bins, PROFILES_OF.index(profile_of)


def check_options(options):
    """what gat-profile does not do, refused before anything is read"""
    enrichment.check_options(options, TOOL, "the point of an anchor is chosen with --anchor-point")
    check_geometry(getattr(options, "bin_size", BIN_SIZE), getattr(options, "half_bins", HALF_BINS), getattr(options, "profile_of", "bases"))
    anchor_position(0, 1, False, getattr(options, "anchor_point", "five-prime"))


def track_profile(track, segs, anchors, workspace, sampler, num_samples, bin_size=BIN_SIZE, half_bins=HALF_BINS, profile_of="bases",
                  random_seed=None, pseudo_count=1.0, ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `anchors` what read_anchors returns.  Returns (rows, the problem's unit count)."""
    from . import _lib
    bin_size, half_bins, mode = check_geometry(bin_size, half_bins, profile_of)
    num_samples, seed, flat, wa, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names, pos, minus, off, n_anchors = anchor_arrays(anchors, contigs)
    if not contigs or not names:
        return [], flat["n_units"]
    ctx = ctx or get_context()
    observed = ctx.list_profile(lists, list_off, 1, pos, minus, off, len(names), len(contigs), bin_size, half_bins, mode)
    P = _lib.Problem(ctx, flat)
    try:
        words = P.sample_profile_enrichment(seed, 0, num_samples, pos, minus, off, len(names), bin_size, half_bins, mode, observed[0])
    finally:
        P.close()
    return rows(track, names, n_anchors, bin_size, half_bins, observed[0], words, num_samples, pseudo_count), flat["n_units"]


def run(segments, anchors, workspace, sampler, num_samples, bin_size=BIN_SIZE, half_bins=HALF_BINS, profile_of="bases",
        random_seed=None, pseudo_count=1.0, qvalue_method="BH", ctx=None):
    """every segment track around every anchor track: the ProfileResults track by track.  random_seed: base of the per-unit
    streams (None: drawn from numpy's global RandomState); every track takes the next num_samples * n_units streams, as
    gat.run hands them out."""
    return enrichment.run_tracks(segments, lambda track, segs, seed: track_profile(
        track, segs, anchors, workspace, sampler, num_samples, bin_size, half_bins, profile_of, seed, pseudo_count, ctx),
        num_samples, random_seed, qvalue_method, TOOL)


def write_results(outfile, results, order="track"):
    """the table, rows ordered by --order (ties by bin)"""
    enrichment.write_results(outfile, results, HEADER, {"track": lambda x: (x.track, x.annotation, x.bin),
                                                        "annotation": lambda x: (x.annotation, x.track, x.bin)}, order)
