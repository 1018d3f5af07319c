"""Plain-Python restatement of the reference's SamplerBruteForce.sample (gat/Engine.pyx:793-871) on the oracle's
RandomState, filter and length_distribution.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the library's brute-force
sampler with it, and tests/test_brute_force_model.py pins it to the reference's own output
(tests/golden/brute_force/kat.json).

The reference's integer types are kept: Position is uint32, PositionDifference int32 (gat/SegmentList.pxd:31-33),
lmin / lmax compare as int32 (gat/SegmentList.pyx:68-77); `remaining` is segments.sum() -- a uint32 sum over ALL segments
-- assigned to an int32.
"""
import json
import os

import numpy as np

from oracle import oracle as O
from shift_model import i32, lmax, lmin, u32

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brute_force", "kat.json")


def load_kats():
    """tests/golden/brute_force/kat.json as dicts: segments, workspace, params (bucket_size, nbuckets, ntries_inner,
    ntries_outer), seed, and sample (pairs) + next, or error (the exception's class name)."""
    d = json.load(open(KAT))
    out = []
    for i, params, seed, flat, nxt, kind in d["cases"]:
        c = dict(segments=[tuple(x) for x in d["shapes"][i][0]], workspace=[tuple(x) for x in d["shapes"][i][1]],
                 params=dict(zip(("bucket_size", "nbuckets", "ntries_inner", "ntries_outer"), params)), seed=seed,
                 kind=kind, error=None, sample=None, next=nxt)
        if isinstance(flat, str):
            c["error"] = flat
        else:
            c["sample"] = list(zip(flat[0::2], flat[1::2]))
        out.append(c)
    return out


class HistogramSampler(object):
    """gat/Engine.pyx:391-435: randint(1, total) looked up in the cumulated histogram, a second draw inside the bucket."""

    def __init__(self, hist, bucket_size):
        self.cdf = np.cumsum(np.asarray(hist, dtype=np.int64))
        self.total = int(self.cdf[-1])
        self.bucket_size = int(bucket_size)

    def sample(self, rng):
        r = rng.randint(1, self.total) if self.total > 1 else 1
        base = int(np.searchsorted(self.cdf, r, side="left")) * self.bucket_size
        if self.bucket_size > 1:
            return base + rng.randint(0, self.bucket_size)
        return base


def bisect_position(cdf, p):
    """utils/gat_utils.c searchsorted with cmpPosition (gat/Engine.pyx:119): the leftmost i with int32(cdf[i] - p) >= 0."""
    lo, hi = 0, len(cdf)
    while lo < hi:
        mid = (lo + hi) // 2
        if i32(cdf[mid] - p) < 0:
            lo = mid + 1
        else:
            hi = mid
    return lo


def sls_sample(rng, workspace, cdf, total, length, notes=None):
    """SegmentListSampler.sample (gat/Engine.pyx:279-348): (start, end, overlap with the chosen piece).  notes, when a
    dict, counts the placements with q < 0 (q_negative), with an overlap smaller than their length (partial_overlap) and
    those of a piece k > 0 whose sampling_start is the previous piece's end (start_at_prev_end)."""
    p = rng.randint(0, total)
    k = bisect_position(cdf, p)
    cs, ce = workspace[k]
    sampling_start = cs - length + 1
    if k > 0:
        if notes is not None and lmax(workspace[k - 1][1], sampling_start) != sampling_start:
            notes["start_at_prev_end"] += 1
        sampling_start = lmax(workspace[k - 1][1], sampling_start)
    q = rng.randint(sampling_start, ce)
    start = u32(lmax(0, q))
    end = u32(q + length)
    overlap = lmax(0, lmin(ce, end) - lmax(cs, start))
    if notes is not None:
        notes["q_negative"] += q < 0
        notes["partial_overlap"] += overlap < length
    return start, end, overlap


EVENTS = ("q_negative", "partial_overlap", "start_at_prev_end", "rej_remaining_only", "rej_hit", "touching")


def new_notes():
    """what sample() notes per call under stats["notes"] (a list, one dict per call): the EVENTS as counts --
    rej_remaining_only: rejections by overlap > remaining where no accepted segment is hit; rej_hit: rejections by a hit;
    touching: accepted segments with an earlier one ending at their start or starting at their end -- and
    hit_lowest (the lowest index, in the order of acceptance, of a hitting entry, per rejection by a hit), hit_only (the
    same where that entry is the only one hit), touching_both (accepted segments touched on both sides), passes ((list
    length when the pass ended, converged) per pass) and words (raw MT19937 outputs consumed)."""
    d = dict((k, 0) for k in EVENTS)
    d.update(hit_lowest=[], hit_only=[], touching_both=0, passes=[], words=0)
    return d


def sample(rng, segments, workspace, bucket_size=1, nbuckets=100000, ntries_inner=100, ntries_outer=10, stats=None):
    """SamplerBruteForce(bucket_size, nbuckets, ntries_inner, ntries_outer).sample(segments, workspace) drawing from rng
    (an oracle RandomState).  Raises ValueError("sampling did not converge") as the reference does.  stats gathers
    restarts (outer passes beyond the first), tries (rejected placements), placed (accepted ones, dropped lists included),
    unconverged and the longest list (list_max); where it holds a list under "notes", a new_notes() dict of the call's
    events is appended to it (none of this changes what is drawn or returned)."""
    if stats is None:
        stats = {}
    for key in ("restarts", "tries", "placed", "unconverged", "list_max"):
        stats.setdefault(key, 0)
    notes = None
    if isinstance(stats.get("notes"), list):
        notes = new_notes()
        stats["notes"].append(notes)
        words0 = rng.ndraws
    segments = [tuple(x) for x in segments]
    workspace = [tuple(x) for x in workspace]
    working = O.aslist(O.filter(segments, workspace)) if segments and workspace else []
    if not working:
        return []
    hist, bucket = O.length_distribution(working, bucket_size, nbuckets)
    hs = HistogramSampler(hist, bucket)
    cdf, total = [], 0
    for s, e in workspace:
        total = u32(total + (e - s))
        cdf.append(u32(total - 1))
    total_sum = i32(sum(e - s for s, e in segments))
    out = []
    outer = ntries_outer
    while outer > 0:
        out = []
        remaining = total_sum
        inner = ntries_inner
        while remaining > 0 and inner > 0:
            length = hs.sample(rng)
            start, end, overlap = sls_sample(rng, workspace, cdf, total, length, notes)
            if overlap > remaining or any(lmin(e, end) - lmax(s, start) > 0 for s, e in out):
                inner -= 1
                stats["tries"] += 1
                if notes is not None:
                    hits = [i for i, (s, e) in enumerate(out) if lmin(e, end) - lmax(s, start) > 0]
                    if overlap > remaining:
                        notes["rej_remaining_only"] += not hits
                    else:
                        notes["rej_hit"] += 1
                        notes["hit_lowest"].append(hits[0])
                        if len(hits) == 1:
                            notes["hit_only"].append(hits[0])
                continue
            if notes is not None:
                sides = any(e == start for _, e in out) + any(s == end for s, _ in out)
                notes["touching"] += sides > 0
                notes["touching_both"] += sides == 2
            out.append((start, end))
            stats["placed"] += 1
            stats["list_max"] = max(stats["list_max"], len(out))
            inner = ntries_inner
            remaining = i32(remaining - overlap)
        if notes is not None:
            notes["passes"].append((len(out), inner > 0))
            notes["words"] = rng.ndraws - words0
        if inner > 0:
            break
        outer -= 1
        if outer > 0:
            stats["restarts"] += 1
    if outer == 0:
        stats["unconverged"] += 1
        raise ValueError("sampling did not converge")
    return sorted(out)


def model_units(flat_units, seed, begin, end, stats=None, **params):
    """the lists of every (sample, unit), sample-major, of units [(segments, workspace)] under the per-unit stream
    contract: unit u of sample s draws from RandomState((seed + s * n_units + u) mod 2^32).  A (sample, unit) that does
    not converge gives None.  stats additionally gathers n_draws (raw MT19937 outputs)."""
    if stats is None:
        stats = {}
    stats.setdefault("n_draws", 0)
    n_units = len(flat_units)
    lists = []
    for s in range(begin, end):
        for u, (segs, ws) in enumerate(flat_units):
            rng = O.RandomState((seed + s * n_units + u) & 0xFFFFFFFF)
            try:
                lists.append(sample(rng, segs, ws, stats=stats, **params))
            except ValueError:
                lists.append(None)
            stats["n_draws"] += rng.ndraws
    return lists
