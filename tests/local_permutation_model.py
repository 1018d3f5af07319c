"""Plain-Python restatement of the reference's SamplerLocalPermutation.sample (gat/Engine.pyx:1117-1229) on CPython's own
random.Random.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the library's local permutation sampler with it, and
tests/test_local_permutation_model.py pins it to the reference's own output (tests/golden/local_permutation/kat.json).

What the reference computes, as opposed to what its docstring describes (DESIGN §5 "k_permute_local"):

* the working segments of a workspace piece (ws, we) are getOverlappingSegments' set (gat/SegmentList.pyx:952-983): from
  the last segment with start <= ws (the first segment when there is none) on, every segment with start <= we -- whether
  or not it reaches the piece;
* `working_segments.min()` / `.max()` (gat/Engine.pyx:1186-1187) are asked of a list built with _add, whose normalized
  flag is 0: their assertions fire inside `cpdef Position` functions, which cannot raise -- the interpreter prints
  "Exception ignored" and they return 0.  So work_start = lmin(0, ws) = 0 and work_end = lmax(0, we) = we: every piece
  is permuted over [0, we), and free = we - sum(lengths) -- negative when the working segments are longer than that,
  where random.randint(0, free) raises ValueError;
* start and end are C ints (PositionDifference) assigned from Python-object arithmetic (`start += points[x] - last`,
  `end = start + lengths[x]`): a value beyond 2^31 - 1 raises OverflowError.  That depends on the draws.

The walk below is the reference's loop line by line; the kernel uses its closed form (segment x of the shuffled list
covers [q_x, q_x + L_x) of [0, we) modulo we, q_x = shift + points[x] + the lengths before it), so a match of the two
checks the closed form as well.
"""
import bisect
import json
import os

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_permutation", "kat.json")
INT_MAX = 2 ** 31 - 1


def load_kats():
    """tests/golden/local_permutation/kat.json as dicts: segments, workspace, seed, sample (pairs) or None with `error`
    (the name of what the reference raised), next (the next getrandbits(32); None where it raised)."""
    d = json.load(open(KAT))
    out = []
    for i, seed, flat, nxt in d["cases"]:
        err = flat if isinstance(flat, str) else None
        out.append(dict(shape=i, segments=[tuple(x) for x in d["shapes"][i][0]], workspace=[tuple(x) for x in d["shapes"][i][1]],
                        seed=seed, sample=None if err else list(zip(flat[0::2], flat[1::2])), error=err, next=nxt))
    return out


def unit_tables(segments, workspace):
    """what problem creation derives for a unit: per ACTIVE workspace piece, in order, (first, n, work_start, work_end,
    free) -- the working segments are segments[first:first + n]; free may be negative (the reference raises)."""
    segments = [tuple(x) for x in segments]
    starts = [s for s, _ in segments]
    out = []
    if not segments:
        return out
    for ws, we in workspace:
        first = max(0, bisect.bisect_right(starts, ws) - 1)
        n = bisect.bisect_right(starts, we) - first
        if n <= 0:
            continue
        total = sum(e - s for s, e in segments[first:first + n])
        out.append((first, n, 0, we, we - total))
    return out


def normalize(pieces):
    """SegmentList.normalize: sorted, overlaps united, adjacent pieces kept apart, empties dropped."""
    out = []
    for s, e in sorted(p for p in pieces if p[0] != p[1]):
        if out and s < out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def _bump(stats, key, by=1):
    if stats is not None and by:
        stats[key] = stats.get(key, 0) + by


def sample(rng, segments, workspace, stats=None):
    """SamplerLocalPermutation().sample(segments, workspace) drawing from rng (a random.Random).  Raises ValueError /
    OverflowError where the reference does.  stats, when given, counts the events of the known-answer conditions."""
    segments = [tuple(x) for x in segments]
    workspace = [tuple(x) for x in workspace]
    tables = unit_tables(segments, workspace)
    if stats is not None:
        starts = [s for s, _ in segments]
        seen_idle = False
        for ws, we in workspace:                         # a piece without working segment in front of an active one
            active = segments and bisect.bisect_right(starts, we) - max(0, bisect.bisect_right(starts, ws) - 1) > 0
            if not active:
                seen_idle = True
            elif seen_idle:
                _bump(stats, "idle_then_active")
                seen_idle = False
        _bump(stats, "adjacent_ws", sum(a[1] == b[0] for a, b in zip(workspace, workspace[1:])))
        used = [0] * len(segments)
        pieces = [w for w in workspace if bisect.bisect_right(starts, w[1]) - max(0, bisect.bisect_right(starts, w[0]) - 1) > 0]
        for (ws, _), (first, n, _, we, free) in zip(pieces if segments else [], tables):
            for i in range(first, first + n):
                used[i] += 1
            _bump(stats, "lone_not_overlapping", n == 1 and not (segments[first][0] < we and segments[first][1] > ws))
            _bump(stats, "n_is_1", n == 1)
            _bump(stats, "n_above_64", n > 64)
            _bump(stats, "free_is_0", free == 0)
            if free >= 0:
                b = free + 1
                _bump(stats, "bound_pow2", b & (b - 1) == 0 and b > 1)
                top = 1 << (b.bit_length() - 1)
                _bump(stats, "bound_above_pow2", 0 < b - top <= top // 16 + 1 and b > 2)
        _bump(stats, "shared_segment", sum(u > 1 for u in used))
        _bump(stats, "near_2_31", any(we > 2 ** 31 - 4096 for _, _, _, we, _ in tables))
    raw = []
    for first, n, work_start, work_end, free in tables:
        lengths = [e - s for s, e in segments[first:first + n]]
        rng.shuffle(lengths)
        points = sorted(rng.randint(0, free) for _ in lengths)        # (free < 0: ValueError, as the reference)
        shift = rng.randint(0, free)
        start, last = work_start + shift, 0
        for x, length in enumerate(lengths):
            start += points[x] - last
            if start > INT_MAX:
                raise OverflowError("value too large to convert to int")
            if start > work_end:
                start = work_start + start - work_end
                _bump(stats, "wrapped_start")
            end = start + length
            if end > INT_MAX:
                raise OverflowError("value too large to convert to int")
            if end < work_end:
                raw.append((start, end))
            else:
                _bump(stats, "end_on_work_end", end == work_end)
                _bump(stats, "start_on_work_end", start == work_end)
                _bump(stats, "wrapped_segment", start < work_end < end)
                raw.append((start, work_end))
                end = work_start + end - work_end
                raw.append((work_start, end))
            start, last = end, points[x]
    out = normalize(raw)
    if stats is not None:
        _bump(stats, "united", len([p for p in raw if p[0] != p[1]]) > len(out))
        _bump(stats, "adjacent_apart", sum(a[1] == b[0] for a, b in zip(out, out[1:])))
        _bump(stats, "empty_result", not out)
        _bump(stats, "raw_pieces", len(raw))
        _bump(stats, "draw_groups", sum(t[1] for t in tables))
    return out
