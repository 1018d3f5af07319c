"""Plain-Python restatement of the reference's SamplerShift.sample (gat/Engine.pyx:1032-1108) on the oracle's
RandomState, normalize, filter and get_insertion_point.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the
library's shift sampler with it, and tests/test_shift_model.py pins it to the reference's own output
(tests/golden/shift/kat.json).

The reference's integer types are kept: Position is uint32, PositionDifference int32
(gat/SegmentList.pxd:31-33), lmin / lmax compare as int32 (gat/SegmentList.pyx:68-77), and every
implicit C conversion between them wraps as it does in the compiled reference.
"""
import json
import math
import os

from oracle import oracle as O

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shift", "kat.json")


def load_kats():
    """tests/golden/shift/kat.json as dicts: segments, workspace, radius, extension, seed, sample (pairs), next."""
    d = json.load(open(KAT))
    return [dict(segments=[tuple(x) for x in d["shapes"][i][0]], workspace=[tuple(x) for x in d["shapes"][i][1]],
                 radius=radius, extension=extension, seed=seed, sample=list(zip(flat[0::2], flat[1::2])), next=nxt)
            for i, radius, extension, seed, flat, nxt in d["cases"]]


def u32(x):
    return x & 0xFFFFFFFF


def i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def lmin(a, b):
    a, b = i32(a), i32(b)
    return a if a < b else b


def lmax(a, b):
    a, b = i32(a), i32(b)
    return a if a > b else b


def _sum(ws):
    return sum(e - s for s, e in ws)


def window(workspace, seg_start, seg_end, radius, extension):
    """the window of one working segment: getOverlappingSegmentsWithRange + truncate (a normalized list of pieces)."""
    length = u32(seg_end - seg_start)
    mid = u32(seg_start + length // 2)
    if extension:
        area = int(extension) // 2
    else:
        area = i32(u32(int(math.floor(length * (radius / 2)))))
    ws_start = lmax(0, u32(mid - area))
    ws_end = lmax(0, u32(mid + area))
    # getOverlappingSegments (gat/SegmentList.pyx:952-1000)
    n = len(workspace)
    pieces = []
    if n:
        idx = O.get_insertion_point(workspace, u32(ws_start), u32(ws_end))
        if idx == n:
            idx -= 1
        elif idx == -1:
            idx = 0
        while idx < n and workspace[idx][0] <= u32(ws_end):
            pieces.append(list(workspace[idx]))
            idx += 1
    # truncate (:1186-1203): unsigned compares against the range
    s0, e0 = u32(ws_start), u32(ws_end)
    for p in pieces:
        if p[1] < s0:
            p[0] = p[1] = 0
        elif p[0] > e0:
            p[0] = p[1] = 0
        else:
            if p[0] < s0:
                p[0] = s0
            if p[1] > e0:
                p[1] = e0
    return [tuple(x) for x in O.aslist(O.normalize(pieces))] if pieces else []


def filled_from_start(ws, start, remainder):
    """SegmentList.getFilledSegmentsFromStart(Position start, PositionDifference remainder) (:1314-1356)."""
    start, remainder = u32(start), i32(remainder)
    if u32(remainder) > _sum(ws):                  # (int against Position: an unsigned compare)
        return list(ws)
    out = []
    n = len(ws)
    idx = O.get_insertion_point(ws, start, u32(start + 1))
    if idx == n:
        idx -= 1
    elif idx == -1:
        idx = 0
    while remainder > 0:
        if ws[idx][1] < start:
            pass
        else:
            start = u32(lmax(ws[idx][0], start))
            end = u32(lmin(ws[idx][1], u32(start + remainder)))
            remainder = i32(remainder - u32(end - start))
            out.append((start, end))
        idx += 1
        if idx == n:
            idx = 0
            start = ws[idx][0]
    return out


def filled_from_end(ws, end, remainder):
    """SegmentList.getFilledSegmentsFromEnd(Position end, PositionDifference remainder) (:1358-1399)."""
    end, remainder = u32(end), i32(remainder)
    if u32(remainder) > _sum(ws):                  # (int against Position: an unsigned compare)
        return list(ws)
    out = []
    n = len(ws)
    idx = O.get_insertion_point(ws, end, u32(end + 1))
    if idx == n:
        idx -= 1
    elif idx == -1:
        idx = 0
    while remainder > 0:
        if ws[idx][0] > end:
            pass
        else:
            end = u32(lmin(ws[idx][1], end))
            start = u32(lmax(ws[idx][0], u32(end - remainder)))
            remainder = i32(remainder - u32(end - start))
            out.append((start, end))
        idx -= 1
        if idx < 0:
            idx = n - 1
            end = ws[idx][1]
    return out


def _fill(fill, ws, x, remainder, stats):
    """one fill, noting in stats how many pieces the widest window taken whole (the remainder beyond its bases) had."""
    if u32(remainder) > _sum(ws):
        stats["fill_all_max"] = max(stats.get("fill_all_max", 0), len(ws))
    return fill(ws, x, remainder)


def random_position(rng, ws, stats):
    """SegmentList.getRandomPosition (:902-917); randint(0, 0) raises ValueError, which the cpdef's C return type turns
    into a printed warning and 0 -- no draw."""
    total = _sum(ws)
    if total == 0:
        stats["empty_windows"] = stats.get("empty_windows", 0) + 1
        return 0
    pos = rng.randint(0, total)
    for s, e in ws:
        l = e - s
        if pos > l:
            pos -= l
        else:
            return s + pos
    raise AssertionError("getRandomPosition ran off the list")


def sample(rng, segments, workspace, radius=2.0, extension=0, stats=None):
    """SamplerShift(radius, extension).sample(segments, workspace) drawing from rng (an oracle RandomState).  stats
    gathers the empty windows, the widest window a fill took whole (fill_all_max) and the most pieces a call put down
    before its normalize (raw_pieces_max)."""
    if stats is None:
        stats = {}
    extension = int(extension)
    segments = [tuple(x) for x in segments]
    workspace = [tuple(x) for x in workspace]
    working = O.aslist(O.filter(segments, workspace)) if segments and workspace else []
    out = []
    for s, e in working:
        length = u32(e - s)
        ws = window(workspace, s, e, radius, extension)
        start = i32(random_position(rng, ws, stats))
        if rng.randint(0, 2):
            end = i32(start + length)
        else:
            end = start
            start = i32(u32(end - length))
        ws_start = i32(ws[0][0]) if ws else 0
        ws_end = i32(ws[-1][1]) if ws else 0
        if start < ws_start:
            remainder = lmin(ws_start - start, length)
            out += _fill(filled_from_start, ws, start, u32(length - remainder), stats)
            out += _fill(filled_from_end, ws, ws_end, remainder, stats)
        elif end > ws_end:
            remainder = lmin(end - ws_end, length)
            out += _fill(filled_from_end, ws, end, u32(length - remainder), stats)
            out += _fill(filled_from_start, ws, ws_start, remainder, stats)
        else:
            out += _fill(filled_from_start, ws, start, length, stats)
    stats["raw_pieces_max"] = max(stats.get("raw_pieces_max", 0), len(out))
    if not out:
        return []
    return [tuple(x) for x in O.aslist(O.normalize(out))]
