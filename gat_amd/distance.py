"""gat-distance: do the segments lie closer to an annotation than chance would put them?

The two counters the reference's to-do list names and never built (doc/contents.rst:78-81: "Closest distance of segment to
annotation", "Closest distance of annotation to segment") -- the test regioneR's mean distance, `bedtools closest -d` and
GenometriCorr's absolute distance make, and the one that matters for sparse annotations (TSSs, CTCF sites, breakpoints),
where the overlap is zero in almost every sample.  Four counters:

    segment-distance      the mean distance from a segment to the nearest interval of the annotation
    segment-nearby        how many segments have one within --max-distance
    annotation-distance   the mean distance from an interval of the annotation to the nearest segment
    annotation-nearby     how many intervals of the annotation have a segment within --max-distance

The distance of [s, e) to a normalized list is 0 where they share a base, else the bases between it and the nearer
neighbour + 1: bookended intervals are at distance 1 (`bedtools closest -d`; include/gat_mi355.h has the definition).
Segments and annotations are both taken to contig level (problem.from_isochores), so distances are genomic and cross isochore
borders.  An interval on a contig where the other side has nothing has no neighbour: it is left out of the mean and of the
count (the word `none`).  The contigs are those the sampler runs on -- the problem's -- for the observed value and the null.

The observed value comes from gat_list_distances on the input segments, the null from gat_sample_distances: the sampler's
batch loop with k_distance behind every batch, so no sampled list comes back to the host.  The rows are ordinary
AnnotatorResults: a fold below 1 on a *-distance counter means closer than expected.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import numpy as np

from . import enrichment
from . import problem
from .engine import AnnotatorResult, get_context

flatten, make_sampler, build_inputs, contig_lists = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs, enrichment.contig_lists
WORDS = ("n", "sum", "near", "none")
SEGMENT_TO_ANNOTATION, ANNOTATION_TO_SEGMENT = 0, 1
# counter -> (direction, which value of a list's words)
COUNTERS = {"segment-distance": (SEGMENT_TO_ANNOTATION, "mean"), "segment-nearby": (SEGMENT_TO_ANNOTATION, "near"),
            "annotation-distance": (ANNOTATION_TO_SEGMENT, "mean"), "annotation-nearby": (ANNOTATION_TO_SEGMENT, "near")}
COUNTER_NAMES = ("segment-distance", "segment-nearby", "annotation-distance", "annotation-nearby")
MAX_DISTANCE = 1000


def values(words, counter):
    """the counter's value of lists whose four sums are words[..., 4]: float64, sum / n (0.0 where n == 0) or near"""
    words = np.asarray(words, dtype=np.int64)
    if COUNTERS[counter][1] == "near":
        return words[..., 2].astype(np.float64)
    n, total = words[..., 0], words[..., 1]
    return np.where(n > 0, total.astype(np.float64) / np.maximum(n, 1), 0.0)


def rows(track, annotations, counter, observed_words, sample_words, pseudo_count=1.0):
    """the result rows of one segment track and one counter: observed_words [n_tracks][4] of the input segments,
    sample_words [samples][n_tracks][4] of the null, annotations: the tracks' names in that order"""
    obs = values(observed_words, counter)
    null = values(sample_words, counter)
    return [AnnotatorResult(track=track, annotation=a, counter=counter, observed=obs[t], samples=null[:, t], pseudo_count=pseudo_count)
            for t, a in enumerate(annotations)]


def check_options(options):
    """what the distance counters do not do, refused before anything is read"""
    enrichment.check_options(options, "gat-distance")


def track_distances(track, segs, annotations, workspace, sampler, counters, num_samples, max_distance=MAX_DISTANCE, random_seed=None,
                    pseudo_count=1.0, ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them, `annotations` the IntervalCollection.  Returns (rows by counter in `counters`' order, the problem's unit count)."""
    from . import _lib
    for c in counters:
        if c not in COUNTERS:
            raise ValueError("unknown counter '%s'" % c)
    max_distance = int(max_distance)
    if not 0 <= max_distance <= 2 ** 32:
        raise ValueError("max_distance %d outside [0, 2^32]" % max_distance)
    num_samples, seed, flat, _, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    names = list(annotations.tracks)
    if not contigs or not names:
        return [[] for _ in counters], flat["n_units"]
    annos, anno_off = contig_lists([problem.from_isochores(annotations[t].asArrays()) for t in names], contigs)
    ctx = ctx or get_context()
    observed, null = {}, {}
    P = _lib.Problem(ctx, flat)
    try:
        for d in sorted(set(COUNTERS[c][0] for c in counters)):
            observed[d] = _lib.list_distances(ctx, lists, list_off, 1, annos, anno_off, len(names), len(contigs), d, max_distance)[0]
            null[d] = P.sample_distances(seed, 0, num_samples, annos, anno_off, len(names), d, max_distance)
    finally:
        P.close()
    return [rows(track, names, c, observed[COUNTERS[c][0]], null[COUNTERS[c][0]], pseudo_count) for c in counters], flat["n_units"]


def run(segments, annotations, workspace, sampler, counters, num_samples, max_distance=MAX_DISTANCE, random_seed=None, pseudo_count=1.0,
        ctx=None):
    """every segment track against every annotation track: the AnnotatorResults in gat.run's order -- counter, track,
    annotation.  random_seed: base of the per-unit streams (None: drawn from numpy's global RandomState); every track takes
    the next num_samples * n_units streams, as gat.run hands them out."""
    seed = int(np.random.randint(0, 2 ** 32)) if random_seed is None else int(random_seed)
    by_counter = [[] for _ in counters]
    for track in segments.tracks:
        per, n_units = track_distances(track, segments[track], annotations, workspace, sampler, counters, num_samples, max_distance,
                                       seed, pseudo_count, ctx)
        seed = (seed + int(num_samples) * int(n_units)) & 0xFFFFFFFF
        for k, r in enumerate(per):
            by_counter[k].extend(r)
    return [r for per in by_counter for r in per]


def observed_format(counters):
    """IO.outputResults' format of the observed column: a mean distance is no integer"""
    return "%6.4f" if any(COUNTERS[c][1] == "mean" for c in counters) else "%i"
