"""The model of gat_sample_coverage (include/gat_mi355.h): lists -> bases / starts / ends / outside.  TEST INFRASTRUCTURE ONLY.

Bin b is [b * bin_size, (b + 1) * bin_size); a contig has n_bins of them.  Every segment [s, e) with e > s adds its overlap
with each bin to `bases`, what lies at or beyond n_bins * bin_size to `outside`, one to `starts` at the bin of s and one to
`ends` at the bin of e - 1 (beyond the last bin: dropped).  Lists need be neither sorted nor disjoint.

coverage() is numpy in int64 with a difference array for the bins a segment covers whole; coverage_naive() walks base by
base and is for tiny inputs.  from_sample() applies coverage() to what Problem.sample returns, contig by contig, in the
layout Problem.sample_coverage returns.
"""
import numpy as np


def _pairs(segments):
    a = np.asarray(segments)
    if a.dtype.names:
        s, e = a["start"].astype(np.int64), a["end"].astype(np.int64)
    else:
        a = a.astype(np.int64).reshape(-1, 2)
        s, e = a[:, 0], a[:, 1]
    keep = e > s
    return s[keep], e[keep]


def coverage(segments, bin_size, n_bins):
    """(bases, starts, ends, outside) of one contig's segments: int64 arrays of n_bins entries and an int."""
    bin_size, n_bins = int(bin_size), int(n_bins)
    s, e = _pairs(segments)
    ext = n_bins * bin_size
    outside = int((np.maximum(e, ext) - np.maximum(s, ext)).sum())
    partial = np.zeros(n_bins + 1, dtype=np.int64)
    diff = np.zeros(n_bins + 2, dtype=np.int64)
    starts = np.zeros(n_bins + 1, dtype=np.int64)
    ends = np.zeros(n_bins + 1, dtype=np.int64)
    np.add.at(starts, np.minimum(s // bin_size, n_bins), 1)
    np.add.at(ends, np.minimum((e - 1) // bin_size, n_bins), 1)
    inside = s < ext
    cs, ce = s[inside], np.minimum(e[inside], ext)
    fb, lb = cs // bin_size, (ce - 1) // bin_size
    one = fb == lb
    np.add.at(partial, fb[one], (ce - cs)[one])
    more = ~one
    np.add.at(partial, fb[more], ((fb + 1) * bin_size - cs)[more])
    np.add.at(partial, lb[more], (ce - lb * bin_size)[more])
    np.add.at(diff, fb[more] + 1, 1)               # whole bins: fb + 1 .. lb - 1
    np.add.at(diff, lb[more], -1)
    bases = partial[:n_bins] + bin_size * np.cumsum(diff)[:n_bins]
    return bases, starts[:n_bins], ends[:n_bins], outside


def coverage_naive(segments, bin_size, n_bins):
    """the same, base by base"""
    bases, starts, ends = (np.zeros(n_bins, dtype=np.int64) for _ in range(3))
    outside = 0
    for s, e in zip(*_pairs(segments)):
        s, e = int(s), int(e)
        for x in range(s, e):
            if x // bin_size < n_bins:
                bases[x // bin_size] += 1
            else:
                outside += 1
        if s // bin_size < n_bins:
            starts[s // bin_size] += 1
        if (e - 1) // bin_size < n_bins:
            ends[(e - 1) // bin_size] += 1
    return bases, starts, ends, outside


def total_length(segments):
    s, e = _pairs(segments)
    return int((e - s).sum())


def from_sample(seg, off, n_contigs, bin_size, n_bins):
    """(bases, starts, ends, outside) over the samples of Problem.sample's (seg, off): list (sample i, contig c) is
    seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]]; the arrays hold contig c's bins at [bin_off[c], bin_off[c + 1])."""
    n_samples = (len(off) - 1) // n_contigs if n_contigs else 0
    out = [[], [], []]
    outside = np.zeros(n_contigs, dtype=np.int64)
    for c in range(n_contigs):
        parts = [seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for i in range(n_samples)]
        lists = np.concatenate(parts) if parts else seg[:0]
        b, s, e, outside[c] = coverage(lists, bin_size, n_bins[c])
        for acc, x in zip(out, (b, s, e)):
            acc.append(x)
    cat = [np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in out]
    return cat[0], cat[1], cat[2], outside
