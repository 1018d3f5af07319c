"""What gat-local, gat-pairs and gat-geneset share (and, as far as it goes, gat-distance): each tests many cells -- (annotation,
bin)s, pairs of annotations, terms -- of every segment track against the sampled null, and the null of a cell comes back from
the device as five integers, WORDS (include/gat_mi355.h has the definition).  Here: the statistics of a row from those five,
the q-values, the options refused, the table, the loop over the segment tracks with its seeds, the start of a track, the
inputs of a run and the scripts' main.  The name of the tool and its wording come in as values; nothing here knows the tools.
"""
import math
import sys
import time

import numpy as np

from . import intervals as iv
from . import problem
from . import stats
from .coverage import SAMPLERS, flatten, make_sampler                # noqa: F401
from .engine import check_sampler, set_device, twoSidedPValueFromCounts

WORDS = ("n_pos", "sum", "sumsq", "n_less", "n_eq")
QVALUE_METHODS = ("BH", "bonferroni", "holm", "hommel", "hochberg", "BY", "none")      # what stats.adjustPValues offers


def bin_statistics(observed, words, num_samples, pseudo_count=1.0):
    """(expected, stddev, fold, pvalue) of one cell from its five words over num_samples samples: the numbers
    AnnotatorResult makes from the row of sample values, without the row.  The radicand of the standard deviation is formed
    in Python integers: S * sumsq and sum * sum pass 2^64."""
    n_pos, total, sumsq, n_less, n_eq = (int(w) for w in words)
    sumsq %= 2 ** 64                          # (the one word that may pass 2^63: it comes in an int64)
    S, observed = int(num_samples), int(observed)
    expected = total / S
    stddev = math.sqrt(S * sumsq - total * total) / S
    fold = (observed + pseudo_count) / (expected + pseudo_count) if expected != 0 else 1.0
    return expected, stddev, fold, twoSidedPValueFromCounts(n_less, n_eq, observed > expected, S)


def check_qvalue_method(method, tool):
    if method not in QVALUE_METHODS:
        raise ValueError("%s: --qvalue-method=%s is not one of %s (stats.adjustPValues)" % (tool, method, ", ".join(QVALUE_METHODS)))


def set_qvalues(results, method, tool):
    """q-values over the rows written, per segment track"""
    check_qvalue_method(method, tool)
    by_track = {}
    for x in results:
        by_track.setdefault(x.track, []).append(x)
    for family in by_track.values():
        for x, q in zip(family, stats.adjustPValues([x.pvalue for x in family], method=method)):
            x.qvalue = float(q)


def check_options(options, tool, points_why="a position list is not an interval list"):
    """what the tool does not do, refused before anything is read"""
    if getattr(options, "conditional", "unconditional") != "unconditional":
        raise NotImplementedError("%s: only --conditional=unconditional (the samples of a generated workspace are not measured)" % tool)
    if getattr(options, "annotations_to_points", None):
        raise NotImplementedError("%s: --annotations-to-points is not supported (%s)" % (tool, points_why))
    if getattr(options, "reference_stream", False):
        raise NotImplementedError("%s: per-unit streams only, not --reference-stream" % tool)


def write_results(outfile, results, header, tie_keys, order="track"):
    """the table, rows ordered by --order; tie_keys: the sort keys of the orders `track` and `annotation`, where rows tie"""
    keys = dict(tie_keys, observed=lambda x: x.observed, fold=lambda x: x.fold, pvalue=lambda x: x.pvalue, qvalue=lambda x: x.qvalue)
    if order not in keys:
        raise ValueError("unknown sort order %s" % order)
    outfile.write("\t".join(header) + "\n")
    for x in sorted(results, key=keys[order]):
        outfile.write(str(x) + "\n")


def run_tracks(segments, track_rows, num_samples, random_seed, qvalue_method, tool):
    """the rows of every segment track, track by track: track_rows(track, segs, seed) -> (rows, the problem's unit count).
    random_seed: base of the per-unit streams (None: drawn from numpy's global RandomState); every track takes the next
    num_samples * n_units streams, as gat.run hands them out.  The q-values are set at the end."""
    check_qvalue_method(qvalue_method, tool)
    seed = int(np.random.randint(0, 2 ** 32)) if random_seed is None else int(random_seed)
    results = []
    for track in segments.tracks:
        per, n_units = track_rows(track, segments[track], seed)
        seed = (seed + int(num_samples) * int(n_units)) & 0xFFFFFFFF
        results.extend(per)
    set_qvalues(results, qvalue_method, tool)
    return results


def contig_lists(per_entity, contigs):
    """(SEG array, CSR offsets) of len(per_entity) x len(contigs) lists, entity-major: per_entity[i] is a dict contig -> SEG
    array (contig level); a contig it lacks is an empty list"""
    lists = [per.get(c, iv.EMPTY) for per in per_entity for c in contigs]
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(a) for a in lists], out=off[1:])
    return (np.concatenate(lists) if off[-1] else iv.EMPTY.copy()), off


def track_start(segs, workspace, sampler, num_samples, random_seed):
    """how the work on one segment track begins: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts
    takes them.  The sampler and num_samples are checked.  Returns (num_samples, the seed -- None: drawn from numpy's global
    RandomState --, the flat problem, the workspace arrays, the problem's contigs, and the segments' contig-level lists over
    them with their offsets: contig_lists)."""
    check_sampler(sampler)
    num_samples = int(num_samples)
    if num_samples < 1:
        raise ValueError("num_samples < 1")
    seed = int(np.random.randint(0, 2 ** 32)) if random_seed is None else int(random_seed)
    flat, sa, wa = flatten(segs, workspace, sampler)
    contigs = list(flat["contig_names"])
    lists, list_off = contig_lists([problem.from_isochores(sa)], contigs)
    return num_samples, seed, flat, wa, contigs, lists, list_off


def build_inputs(options):
    """segments, annotations and the workspace of a run as gat-run.py prepares them (IO.buildSegments / IO.applyIsochores)"""
    from . import io as IO
    segments, annotations, workspaces, isochores = IO.buildSegments(options)
    workspace = IO.applyIsochores(segments, annotations, workspaces, options, isochores,
                                  truncate_segments_to_workspace=options.truncate_segments_to_workspace,
                                  truncate_workspace_to_annotations=options.truncate_workspace_to_annotations,
                                  restrict_workspace=options.restrict_workspace)
    return segments, annotations, workspace


def read_inputs(options):
    """what a script's run call takes from the options: segments, annotations, workspace (build_inputs) and the sampler, with
    the device of --device set"""
    segments, annotations, workspace = build_inputs(options)
    sampler = make_sampler(options)
    set_device(options.device)
    return segments, annotations, workspace, sampler


def main(tool, argv, options, run):
    """a script's main behind its parser and its own checks: --stdout and --log opened, the banner, numpy seeded with
    --random-seed, results = run(options, log) -- log(line) writes a `# ` line at --verbose >= 1, else None --, the tool
    module's table and the closing line"""
    tstart = time.time()
    close_out = False
    if options.stdout and options.stdout != "-":
        options.stdout = open(options.stdout, "w")
        close_out = True
    else:
        options.stdout = sys.stdout
    log = open(options.stdlog, "a") if options.stdlog else options.stdout
    if options.loglevel >= 1:
        log.write("# output generated by %s\n# job started at %s\n" % (" ".join(argv), time.asctime()))
    if options.random_seed is not None:
        np.random.seed(options.random_seed)
    results = run(options, (lambda line: log.write("# %s\n" % line)) if options.loglevel >= 1 else None)
    tool.write_results(options.stdout, results, options.output_order)
    if options.loglevel >= 1:
        log.write("# job finished in %i seconds at %s\n" % (time.time() - tstart, time.asctime()))
    if close_out:
        options.stdout.close()
    if options.stdlog:
        log.close()
    return 0
