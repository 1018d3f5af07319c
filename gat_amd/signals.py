"""gat-signal: is a quantitative track -- conservation, GC content, a ChIP or ATAC signal, a methylation level, a recombination
rate -- higher (or lower) over the segments than chance would give?

The annotation of every other tool here is a set of intervals, present or absent; a signal track is a bedGraph: pieces with a
value each.  Thresholding it into intervals throws the values away.  Four counters, per (segment track, signal track):

    signal-mean      the mean value over the bases of the segments that carry one: sum / covered
    signal-sum       the sum of the values over those bases
    signal-covered   how many bases of the segments carry a value
    signal-hit       how many segments have a base that carries a value

The device works in integers: a value v is quantised to q = rint(v * scale) (round half to even; --signal-scale, default
1000), a signed 32-bit integer, and the four words n, covered, hit, sum of a segment list (include/gat_mi355.h has the
definition) are exact.  signal-mean and signal-sum divide by the scale again.  The pieces are taken as the file gives them, not
cut to the workspace; contigs the problem lacks are ignored.  Segments are taken to contig level (problem.from_isochores).

The observed value comes from gat_list_signal on the input segments, the null from gat_sample_signal: the sampler's batch loop
with k_signal behind every batch, so no sampled list comes back to the host.  The rows are ordinary AnnotatorResults.  fold and
l2fold are meaningful for non-negative signals only -- AnnotatorResult prints -inf for the l2fold of a non-positive fold; the
p-value is valid either way.  The pseudo count defaults to 0 here: a mean is not a count.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without sharding.
"""
import collections
import os

import numpy as np

from . import enrichment
from . import intervals as iv
from .engine import AnnotatorResult, get_context

flatten, make_sampler = enrichment.flatten, enrichment.make_sampler
WORDS = ("n", "covered", "hit", "sum")
COUNTER_NAMES = ("signal-mean", "signal-sum", "signal-covered", "signal-hit")
SCALE = 1000.0
PSEUDO_COUNT = 0.0
Q_MAX = 2 ** 31 - 1
HEADER_PREFIXES = ("track", "browser", "#")

# one signal track: name, and per contig (SEG array of the pieces -- sorted, disjoint, none empty --, int32 values beside them)
Track = collections.namedtuple("Track", ("name", "pieces"))


def track_name(filename):
    """a file's track: its basename without .gz and without the last extension"""
    base = os.path.basename(filename)
    if base.endswith(".gz"):
        base = base[:-3]
    return os.path.splitext(base)[0]


def quantise(values, scale=SCALE):
    """q = rint(float64(value) * scale) as int32; ValueError for a value that is not finite or an |q| beyond 2^31 - 1"""
    q = np.rint(np.asarray(values, dtype=np.float64) * float(scale))
    if not np.all(np.isfinite(q)):
        raise ValueError("a signal value is not finite")
    if len(q) and np.abs(q).max() > Q_MAX:
        raise ValueError("a signal value times the scale %g is beyond 2^31 - 1 in size: %g" % (float(scale), q[np.abs(q).argmax()]))
    return q.astype(np.int32)


def read_bedgraph(filename, scale=SCALE):
    """one bedGraph file -> Track: four columns (contig, start, end, value), lines that start with `track`, `browser` or `#`
    skipped, .gz through IO.openFile.  Zero-length pieces are dropped; overlapping pieces are a ValueError naming the file and
    the contig."""
    from . import io as IO
    per = collections.OrderedDict()
    with IO.openFile(filename) as f:
        for number, line in enumerate(f, 1):
            if not line.strip() or line.startswith(HEADER_PREFIXES):
                continue
            data = line.split()
            if len(data) < 4:
                raise ValueError("%s:%d: a bedGraph line has four columns: contig, start, end, value" % (filename, number))
            start, end = int(data[1]), int(data[2])
            if end < start or start < 0 or end > 2 ** 32 - 1:
                raise ValueError("%s:%d: start %d, end %d" % (filename, number, start, end))
            if end > start:
                per.setdefault(data[0], []).append((start, end, float(data[3])))
    pieces = collections.OrderedDict()
    for contig, rows in per.items():
        a = np.array(rows, dtype=np.float64).reshape(-1, 3)
        order = np.argsort(a[:, 0], kind="stable")
        start, end = a[order, 0].astype(np.int64), a[order, 1].astype(np.int64)
        if np.any(start[1:] < end[:-1]):
            raise ValueError("%s: overlapping pieces on contig %s" % (filename, contig))
        try:
            q = quantise(a[order, 2], scale)
        except ValueError as e:
            raise ValueError("%s: contig %s: %s" % (filename, contig, e))
        pieces[contig] = (iv.make(start, end), q)
    return Track(track_name(filename), pieces)


def read_tracks(filenames, scale=SCALE):
    """the tracks of --signal in the order given; two files of one name are a ValueError"""
    tracks, seen = [], {}
    for fn in filenames:
        name = track_name(fn)
        if name in seen:
            raise ValueError("signal files %s and %s are both track '%s'" % (seen[name], fn, name))
        seen[name] = fn
        tracks.append(read_bedgraph(fn, scale))
    return tracks


def piece_lists(tracks, contigs):
    """(SEG array, int32 values, CSR offsets) of len(tracks) x len(contigs) piece lists, track-major; a contig a track lacks
    is an empty list"""
    segs, off = enrichment.contig_lists([{c: p[0] for c, p in t.pieces.items()} for t in tracks], contigs)
    vals = [t.pieces[c][1] for t in tracks for c in contigs if c in t.pieces]
    return segs, (np.concatenate(vals) if vals else np.zeros(0, dtype=np.int32)).astype(np.int32), off


def values(words, counter, scale=SCALE):
    """the counter's value of lists whose four sums are words[..., 4]: float64"""
    words = np.asarray(words, dtype=np.int64)
    if counter == "signal-covered":
        return words[..., 1].astype(np.float64)
    if counter == "signal-hit":
        return words[..., 2].astype(np.float64)
    covered, total = words[..., 1], words[..., 3].astype(np.float64)
    if counter == "signal-sum":
        return total / float(scale)
    if counter == "signal-mean":
        return np.where(covered > 0, total / np.maximum(covered, 1) / float(scale), 0.0)
    raise ValueError("unknown counter '%s'" % counter)


def rows(track, names, counter, observed_words, sample_words, scale=SCALE, pseudo_count=PSEUDO_COUNT):
    """the result rows of one segment track and one counter: observed_words [n_tracks][4] of the input segments,
    sample_words [samples][n_tracks][4] of the null, names: the signal tracks' in that order"""
    obs = values(observed_words, counter, scale)
    null = values(sample_words, counter, scale)
    return [AnnotatorResult(track=track, annotation=a, counter=counter, observed=obs[t], samples=null[:, t], pseudo_count=pseudo_count)
            for t, a in enumerate(names)]


def check_options(options):
    """what gat-signal does not do, refused before anything is read"""
    enrichment.check_options(options, "gat-signal", "a signal track has no positions")
    for name in ("truncate_workspace_to_annotations", "restrict_workspace", "truncate_segments_to_workspace"):
        if getattr(options, name, False):
            raise NotImplementedError("gat-signal: --%s is not supported (there are no annotation intervals; the segments are filtered "
                                      "by the workspace)" % name.replace("_", "-"))
    if not getattr(options, "signal_files", None):
        raise ValueError("gat-signal: please specify at least one --signal file")
    scale = float(getattr(options, "signal_scale", SCALE))
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("gat-signal: --signal-scale %r is not a positive number" % scale)


def build_inputs(options):
    """segment tracks and the workspace as gat-coverage prepares them (no annotation intervals are read)"""
    from . import coverage
    return coverage.build_inputs(options)


def track_signal(track, segs, tracks, workspace, sampler, counters, num_samples, scale=SCALE, random_seed=None,
                 pseudo_count=PSEUDO_COUNT, ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `tracks` the signal Tracks.  Returns (rows by counter in `counters`' order, the problem's unit count)."""
    from . import _lib
    for c in counters:
        if c not in COUNTER_NAMES:
            raise ValueError("unknown counter '%s'" % c)
    num_samples, seed, flat, _, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names = [t.name for t in tracks]
    if not contigs or not names:
        return [[] for _ in counters], flat["n_units"]
    pieces, vals, piece_off = piece_lists(tracks, contigs)
    ctx = ctx or get_context()
    P = _lib.Problem(ctx, flat)
    try:
        observed = _lib.list_signal(ctx, lists, list_off, 1, pieces, vals, piece_off, len(names), len(contigs))[0]
        null = P.sample_signal(seed, 0, num_samples, pieces, vals, piece_off, len(names))
    finally:
        P.close()
    return [rows(track, names, c, observed, null, scale, pseudo_count) for c in counters], flat["n_units"]


def run(segments, tracks, workspace, sampler, counters, num_samples, scale=SCALE, random_seed=None, pseudo_count=PSEUDO_COUNT, ctx=None):
    """every segment track against every signal track: the AnnotatorResults in gat.run's order -- counter, track, signal.
    random_seed: base of the per-unit streams (None: drawn from numpy's global RandomState); every track takes the next
    num_samples * n_units streams, as gat.run hands them out."""
    seed = int(np.random.randint(0, 2 ** 32)) if random_seed is None else int(random_seed)
    by_counter = [[] for _ in counters]
    for track in segments.tracks:
        per, n_units = track_signal(track, segments[track], tracks, workspace, sampler, counters, num_samples, scale, seed, pseudo_count, ctx)
        seed = (seed + int(num_samples) * int(n_units)) & 0xFFFFFFFF
        for k, r in enumerate(per):
            by_counter[k].extend(r)
    return [r for per in by_counter for r in per]


def observed_format(counters):
    """IO.outputResults' format of the observed column: a mean or a sum of values is no integer"""
    return "%6.4f" if any(c in ("signal-mean", "signal-sum") for c in counters) else "%i"
