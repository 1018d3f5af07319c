"""gat-compare: significance of fold-change differences between annotations of one run, or between runs
(scripts/gat-compare.py of the reference), from the count files --output-counts-pattern writes.

For a pair (data1, data2) of result rows the reference forms, sample by sample (scripts/gat-compare.py:214-231),

    fc1 = data1.observed / (data1.samples + pseudo_count) + 0.0001
    fc2 = data2.observed / (data2.samples + pseudo_count) + 0.0001
    sampled = log(fc1 / fc2) + (data2.fold - data1.fold)

and builds an AnnotatorResult from it with observed = data2.fold - data1.fold.  One file of 1 000 annotations is 499 500
such rows; here the rows are formed and reduced on the device (k_compare_rows + k_null_stats, gat_compare_stats) from the
count matrices uploaded once per file, and a result carries the device's statistics -- its transformed row is computed
with numpy only when somebody asks for `.samples`.  `compare_numpy` is the same thing on the host, in the reference's
own numpy operations: the path of small inputs, of the rare pairs with a non-finite sample, and the model the GPU tests
compare against.
"""
import collections
import itertools
import os

import numpy as np

from .engine import AnnotatorResult, get_context

# total transformed values (pairs x samples) from which the device is used when GAT_DEVICE_STATS does not say: below it the
# upload and the launches cost more than numpy does (and no device is needed at all).  DESIGN.md section 5 "k_null_stats"
# quotes the same figure for run().
DEVICE_MIN_VALUES = 2 * 10 ** 6

Pair = collections.namedtuple("Pair", "file1 file2 data1 data2 track annotation")


def transformed_row(data1, data2, pseudo_count):
    """(delta, the sampled fold-change differences) of a pair: scripts/gat-compare.py:214-231, operation for operation."""
    with np.errstate(divide="ignore", invalid="ignore"):
        fold_changes1 = data1.observed / (data1.samples + pseudo_count)
        fold_changes2 = data2.observed / (data2.samples + pseudo_count)
        fold_changes1 += 0.0001
        fold_changes2 += 0.0001
        delta_fold = data2.fold - data1.fold
        return delta_fold, np.log(fold_changes1 / fold_changes2) + delta_fold


class _LazyRow(object):
    """the transformed row of a pair for a result built from the device's statistics: AnnotatorResult keeps it as it is
    and turns it into an array (numpy, on the host) only when its samples are asked for"""
    __slots__ = ("data1", "data2", "pseudo_count")

    def __init__(self, data1, data2, pseudo_count):
        self.data1, self.data2, self.pseudo_count = data1, data2, pseudo_count

    def __len__(self):
        return self.data1.nsamples

    def __array__(self, dtype=None, copy=None):
        row = transformed_row(self.data1, self.data2, self.pseudo_count)[1]
        return row if dtype is None else row.astype(dtype, copy=False)


def pairs_of(all_results):
    """the pairs gat-compare.py compares, in its order.  One file: itertools.combinations of its results (one segment
    track only); several: for every combination of two files, the shared tracks in sorted order and for each the shared
    annotations -- which the reference walks in the order of a Python set, i.e. in no defined order; they are SORTED here
    (the table is re-ordered by --order anyway)."""
    pairs = []
    if len(all_results) == 1:
        results = list(all_results[0])
        if len(set(x.track for x in results)) != 1:
            raise NotImplementedError("multiple segments of interest")
        for data1, data2 in itertools.combinations(results, 2):
            pairs.append(Pair(0, 0, data1, data2, data1.annotation, data2.annotation))
        return pairs
    for index1, index2 in itertools.combinations(range(len(all_results)), 2):
        aa, bb = collections.defaultdict(dict), collections.defaultdict(dict)
        for x in all_results[index1]:
            aa[x.track][x.annotation] = x
        for x in all_results[index2]:
            bb[x.track][x.annotation] = x
        for track in sorted(set(aa.keys()).intersection(bb.keys())):
            for annotation in sorted(set(aa[track].keys()).intersection(bb[track].keys())):
                pairs.append(Pair(index1, index2, aa[track][annotation], bb[track][annotation], track, annotation))
    return pairs


def numpy_result(pair, pseudo_count):
    """the result of one pair as the reference's script builds it: the transformed row, then AnnotatorResult's numpy"""
    delta, row = transformed_row(pair.data1, pair.data2, pseudo_count)
    with np.errstate(invalid="ignore"):
        return AnnotatorResult(pair.track, pair.annotation, "na", 0.0 + delta, row, reference=None, pseudo_count=0)


def compare_numpy(all_results, pseudo_count=1.0):
    """compare() on the host alone, as the reference's script computes it."""
    return [numpy_result(p, pseudo_count) for p in pairs_of(all_results)]


def _check_rows(all_results):
    """every file's rows have one length (they become a matrix)"""
    for k, results in enumerate(all_results):
        lengths = set(x.nsamples for x in results)
        if len(lengths) > 1:
            raise ValueError("counts file %d: rows of %s samples" % (k, " / ".join(str(n) for n in sorted(lengths))))


def _device_wanted(n_values):
    """GAT_DEVICE_STATS=1 / 0 forces / forbids the device as it does for run(); otherwise from DEVICE_MIN_VALUES up, when this
    numpy sums the way k_null_stats restates"""
    from . import _device_stats_wanted
    if os.environ.get("GAT_DEVICE_STATS") is not None:
        return _device_stats_wanted(n_values)
    return n_values >= DEVICE_MIN_VALUES and _device_stats_wanted(n_values)


def device_stats(all_results, pairs, pseudo_count, ctx):
    """[n_pairs][8] of gat_compare_stats for `pairs`: mean, stddev, the interval's two values, samples below / equal to
    delta, the number of non-finite samples, 0.  Every file's rows go to the device once, as a float64 matrix."""
    out = np.zeros((len(pairs), 8), dtype=np.float64)
    index = [dict((id(x), i) for i, x in enumerate(results)) for results in all_results]
    groups = collections.OrderedDict()
    for k, p in enumerate(pairs):
        groups.setdefault((p.file1, p.file2), []).append(k)
    dev = {}
    try:
        for f in sorted(set(f for key in groups for f in key)):
            m = np.ascontiguousarray(np.stack([x.samples for x in all_results[f]]), dtype=np.float64)
            dev[f] = (ctx.alloc(m.nbytes), m.shape[0], m.shape[1])
            ctx.h2d(dev[f][0], m)
        for (f1, f2), ks in groups.items():
            (pa, na, sa), (pb, nb, sb) = dev[f1], dev[f2]
            if sa != sb:
                raise ValueError("counts files %d and %d: rows of %d / %d samples" % (f1, f2, sa, sb))
            sel = [pairs[k] for k in ks]
            out[ks] = ctx.compare_stats(pa, na, pb, nb, sa,
                                        [index[f1][id(p.data1)] for p in sel], [index[f2][id(p.data2)] for p in sel],
                                        [p.data1.observed for p in sel], [p.data2.observed for p in sel],
                                        [p.data2.fold - p.data1.fold for p in sel], pseudo_count)
    finally:
        for ptr, _, _ in dev.values():
            ctx.free(ptr)
    return out


def compare(all_results, pseudo_count=1.0, ctx=None):
    """The AnnotatorResult list of gat-compare.py for `all_results`, one list of results per counts file as fromCounts
    returns them (pairs_of says which pairs, in which order; the shared annotations of two files are walked SORTED, where
    the reference walks a set).  Every result has observed = data2.fold - data1.fold, counter "na", no reference and a
    pseudo count of 0.  From DEVICE_MIN_VALUES transformed values up (GAT_DEVICE_STATS=1: always, =0: never) the statistics
    come from the device and no transformed row exists on the host until a result's `.samples` is read; a pair with a
    non-finite sample (pseudo_count = 0 against a zero count) is recomputed with numpy."""
    all_results = [list(r) for r in all_results]
    _check_rows(all_results)
    pairs = pairs_of(all_results)
    if not pairs:
        return []
    if not _device_wanted(sum(p.data1.nsamples for p in pairs)):
        return [numpy_result(p, pseudo_count) for p in pairs]
    stats = device_stats(all_results, pairs, pseudo_count, ctx or get_context())
    results = []
    for p, st in zip(pairs, stats.tolist()):
        if st[6] != 0:
            results.append(numpy_result(p, pseudo_count))
            continue
        results.append(AnnotatorResult(p.track, p.annotation, "na", 0.0 + (p.data2.fold - p.data1.fold),
                                       _LazyRow(p.data1, p.data2, pseudo_count), reference=None, pseudo_count=0,
                                       _stats=tuple(st[:6])))
    return results
