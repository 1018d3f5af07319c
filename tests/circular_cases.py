"""Units of the SamplerCircular tests (tests/test_circular_gpu.py) and of the circular rows of every list consumer's tests.
TEST INFRASTRUCTURE ONLY.

The unit builders of the sampler's own tests, the dozen units whose lists have what a consumer can get wrong (touching
pieces, lists longer than the unit has segments, pieces from beyond the wrap first, empty lists), the units whose workspace
straddles 2^31 and reaches 2^32 - 1, and the model's lists in the layout of Problem.sample.  tests/test_circular_cases_model.py
asserts on the model that the lists have those properties for the seed and the samples the GPU tests use.
"""
import random

import numpy as np

import circular_model as M
from oracle import oracle as O

CIRCULAR = 6
SEED, SAMPLES = 77, 12                  # what the consumers' sampler tests draw


# ---- the unit builders of tests/test_circular_gpu.py ------------------------------------------------------------------------
def rand_norm(r, n, span, maxlen, start=0):
    """up to n separated, sorted pieces in [start, span) of length at most maxlen."""
    pts = sorted(r.sample(range(start, span), 2 * n))
    return [(pts[2 * i], min(pts[2 * i + 1], pts[2 * i] + maxlen)) for i in range(n) if pts[2 * i + 1] > pts[2 * i]]


def units_flat(units):
    """one contig per unit, no isochores, no annotations: the sampler alone.  A unit without segments or workspace is
    skipped: it carries contig -1."""
    def cat(lists):
        out = np.zeros(sum(len(x) for x in lists), dtype=O.SEG)
        k = 0
        for x in lists:
            for s, e in x:
                out[k] = (s, e)
                k += 1
        return out

    def off(lists):
        return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)

    segs, ws = [s for s, _ in units], [w for _, w in units]
    live = [len(s) > 0 and len(w) > 0 for s, w in units]
    contig = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    return dict(n_units=len(units), segs=cat(segs), seg_off=off(segs), ws=cat(ws), ws_off=off(ws), unit_contig=contig,
                n_contigs=int(sum(live)), merge_contigs=0, n_tracks=0, annos=np.zeros(0, dtype=O.SEG),
                anno_off=np.zeros(1, np.int64), cws_nseg=np.array([len(w) for w, k in zip(ws, live) if k], np.int64),
                sampler=CIRCULAR)


def unit_of_n(r, n, frag):
    """a unit of exactly n working intervals; frag: a workspace of short pieces, so that intervals are cut"""
    segs = [(10 + 7 * i, 10 + 7 * i + r.choice((1, 2, 5))) for i in range(n)]
    top = 10 + 7 * n + 20
    if frag:
        ws, x = [], 0
        while x < top:
            ln = r.choice((3, 9, 16, 40))
            ws.append((x, min(top, x + ln)))
            x += ln + r.choice((0, 0, 1))          # (gaps of one base never swallow a whole segment start..end run)
    else:
        ws = [(0, top)]
    n_iv = len(M.linear_intervals(segs, ws))
    return (segs, ws), n_iv


EDGE_WS = [(10, 20), (25, 30), (30, 31), (40, 60)]               # Wsum 36, touching pieces, a piece of one base
EDGE_SEGS = [(12, 15), (18, 27), (50, 60)]                       # linear [2, 5), [8, 12), [26, 36): the last ends at Wsum


# ---- what the consumers get ---------------------------------------------------------------------------------------------------
def crumbs(r, n_pieces):
    """a workspace of n_pieces pieces of one to five bases, four in ten touching the one before"""
    ws, x = [], 3
    for _ in range(n_pieces):
        ln = r.randint(1, 5)
        ws.append((x, x + ln))
        x += ln + (0 if r.random() < 0.4 else r.randint(1, 4))
    return ws


def roomy(r, n, max_len=40):
    """n segments of 1..max_len bases in a small part of a workspace of four pieces, two of them touching"""
    span = 60 * max_len * n + 500
    segs = rand_norm(r, n, span, max_len)
    cut = sorted(r.sample(range(100, span - 100), 4))
    return segs, [(0, cut[0]), (cut[0] + 7, cut[1]), (cut[2], cut[3]), (cut[3], span)]


EDGE, FILLED, CRUMBS, WAVE_65, MISSED, WSUM_ONE = 0, 1, 2, 4, 6, 7          # where consumer_units() holds what


def consumer_units():
    """a dozen small units, one contig each.  Their lists under (SEED, SAMPLES) hold touching pieces, more pieces than the
    unit has segments, pieces from beyond the wrap at the workspace's first base, and nothing at all (MISSED)."""
    r = random.Random(0xC1C)
    ws_crumbs = crumbs(r, 260)
    top = ws_crumbs[-1][1]
    long_segs = [(5, top // 5), (top // 4, top // 4 + 1), (top // 3, top // 2 + 60), (top - 150, top - 2)]
    return [
        (EDGE_SEGS, EDGE_WS),
        ([(90, 200)], [(100, 110)]),                                           # one piece filled by one segment
        (long_segs, ws_crumbs),                                                # four segments over dozens of pieces each
        ([(2, 9), (40, 300), (310, 311)], crumbs(r, 120)),
        unit_of_n(r, 65, False)[0],                                            # two wave steps
        unit_of_n(r, 65, True)[0],
        ([(500, 510)], [(0, 100)]),                                            # the segments miss the workspace: empty lists
        ([(5, 9)], [(7, 8)]),                                                  # Wsum == 1: no draw, the working list
        ([(4, 31), (60, 61), (100, 140), (199, 203)], [(2 * i, 2 * i + 1) for i in range(90)] + [(200, 201), (201, 202), (202, 203)]),
        ([(0, 50), (70, 75)], [(0, 30), (30, 60), (60, 90), (90, 120)]),       # touching pieces all the way
        roomy(r, 7),
        roomy(r, 40),
    ]


TWO_31, TOP = 2 ** 31, 2 ** 32 - 1


def wide_units():
    """units whose workspace straddles 2^31 and reaches 2^32 - 1, with segments on both sides: the sign bit of a 32-bit
    coordinate flips inside one list.  Only a problem without tracks and isochore keys takes them."""
    return [
        ([(TWO_31 - 4000, TWO_31 - 3000), (TWO_31 - 5, TWO_31 + 100), (TWO_31 + 3000, TWO_31 + 3500), (TOP - 40, TOP - 20)],
         [(TWO_31 - 5000, TWO_31 - 1000), (TWO_31 - 10, TWO_31 + 4000), (TOP - 49, TOP)]),
        ([(10, 300), (TWO_31 - 1, TWO_31 + 1), (TOP - 500, TOP)],
         [(0, 1000), (TWO_31 - 1, TWO_31 + 1), (TOP - 1000, TOP)]),
        ([(TWO_31 - 2900, TWO_31 - 2000), (TWO_31 - 7, TWO_31), (TWO_31, TWO_31 + 9), (TWO_31 + 2500, TWO_31 + 2999)],
         [(TWO_31 - 3000, TWO_31), (TWO_31, TWO_31 + 3000)]),                 # two pieces that touch at 2^31
    ]


# ---- the model's lists as Problem.sample returns them ---------------------------------------------------------------------------
def contig_lists(flat, unit_lists, S):
    """the (sample, unit) lists as (sample, contig) lists: a contig's units one after the other, merge(0)d when the problem's
    keys carry isochores -- what k_contig leaves"""
    n, nc = int(flat["n_units"]), int(flat["n_contigs"])
    lists = []
    for s in range(S):
        contig = [[] for _ in range(nc)]
        for u in range(n):
            c = int(flat["unit_contig"][u])
            if c >= 0:
                contig[c] += unit_lists[s * n + u]
        if int(flat["merge_contigs"]):
            contig = [O.aslist(O.merge(sorted(x), 0)) if x else [] for x in contig]
        lists += contig
    return lists


def as_arrays(lists):
    """lists of (start, end) -> (SEG array, offsets)"""
    cat = np.zeros(sum(len(x) for x in lists), dtype=O.SEG)
    k = 0
    for x in lists:
        for a, b in x:
            cat[k] = (a, b)
            k += 1
    return cat, np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)


def model_sample(flat, seed, s0, s1, unit_level=False):
    """what Problem.sample(seed, s0, s1, unit_level) returns for a circular problem, from tests/circular_model.py"""
    unit_lists, _ = M.model_units(flat, seed, s0, s1)
    return as_arrays(unit_lists if unit_level else contig_lists(flat, unit_lists, s1 - s0))


def dense_isochore_problem():
    """two contigs of two isochore classes each, the classes' workspace pieces interleaved and mostly filled by segments: a
    rotated piece that ends at a border of one unit meets the piece that begins there in the other, and the contig list
    unites what the unit lists keep apart"""
    from collections import OrderedDict
    from gat_amd import problem

    def seg(pairs):
        a = np.zeros(len(pairs), dtype=O.SEG)
        for i, p in enumerate(pairs):
            a[i] = p
        return a
    ws = OrderedDict([("c1.lo", [(0, 30), (60, 90), (120, 150)]), ("c1.hi", [(30, 60), (90, 120)]),
                      ("c2.lo", [(10, 40)]), ("c2.hi", [(40, 50), (50, 70)])])
    segs = OrderedDict([("c1.lo", [(2, 29), (61, 88), (125, 150)]), ("c1.hi", [(31, 59), (95, 118)]),
                        ("c2.lo", [(10, 38)]), ("c2.hi", [(41, 69)])])
    flat = problem.flatten_units(OrderedDict((k, seg(v)) for k, v in segs.items()), OrderedDict((k, seg(v)) for k, v in ws.items()), [])
    flat["sampler"] = CIRCULAR
    return flat
