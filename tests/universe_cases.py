"""Units and problems of the SamplerUniverse tests (tests/test_universe_gpu.py).  TEST INFRASTRUCTURE ONLY.

A unit is (segments, workspace pieces); the segments of a unit built here are members of its universe -- whole pieces --
unless a builder says otherwise.
"""
import collections
import random

import numpy as np

import circular_cases as CIRC
from oracle import oracle as O

UNIVERSE = 7


def pieces(r, m, start=0):
    """m workspace pieces of 1..9 bases, three in ten touching the one before"""
    ws, x = [], start
    for _ in range(m):
        ln = r.randint(1, 9)
        ws.append((x, x + ln))
        x += ln + (0 if r.random() < 0.3 else r.randint(1, 6))
    return ws


def unit_of(r, m, k, hit=None, start=0):
    """a universe of m pieces of which k (or the indices `hit`) are the segments"""
    ws = pieces(r, m, start)
    hit = sorted(r.sample(range(m), k)) if hit is None else sorted(hit)
    return [ws[h] for h in hit], ws


def units_flat(units):
    return dict(CIRC.units_flat(units), sampler=UNIVERSE)


def seg_array(pairs):
    a = np.zeros(len(pairs), dtype=O.SEG)
    for i, p in enumerate(pairs):
        a[i] = p
    return a


def isochore_problem():
    """three contigs of two or three isochore classes each, the classes' pieces interleaved (touching ones among them, so that
    the contig list unites pieces of two units); one class without a hit piece, one with every piece hit"""
    from gat_amd import problem
    r = random.Random(0x150)
    ws, segs = collections.OrderedDict(), collections.OrderedDict()
    for contig, classes, n in (("c1", ("lo", "mid", "hi"), 90), ("c2", ("lo", "hi"), 41), ("c3", ("lo", "hi"), 12)):
        all_pieces = pieces(r, n, start=r.randint(0, 50))
        for j, cls in enumerate(classes):
            mine = all_pieces[j::len(classes)]
            key = "%s.%s" % (contig, cls)
            ws[key] = mine
            if key == "c3.hi":
                segs[key] = [(mine[-1][1] + 100, mine[-1][1] + 120)]          # beyond the universe: k == 0
            elif key == "c2.lo":
                segs[key] = list(mine)                                         # k == m
            else:
                segs[key] = sorted(r.sample(mine, max(1, len(mine) // 3)))
    flat = problem.flatten_units(collections.OrderedDict((k, seg_array(v)) for k, v in segs.items()),
                                 collections.OrderedDict((k, seg_array(v)) for k, v in ws.items()), [])
    flat["sampler"] = UNIVERSE
    return flat


def peak_config():
    """a small peak-set problem for run(): per contig a universe of 40-70 separated candidate regions, a quarter of them the
    segments, three annotation tracks that cover some candidates whole, cut others and miss the rest"""
    r = random.Random(0xBEA)
    contigs = collections.OrderedDict([("chrA", 70), ("chrB", 55), ("chrC", 40)])
    workspace, segments = collections.OrderedDict(), collections.OrderedDict()
    tracks = [("t%d" % i, collections.OrderedDict()) for i in range(3)]
    for contig, n in contigs.items():
        ws, x = [], r.randint(0, 300)
        for _ in range(n):
            ln = r.randint(150, 600)
            ws.append((x, x + ln))
            x += ln + r.randint(50, 2000)
        workspace[contig] = seg_array(ws)
        segments[contig] = seg_array(sorted(r.sample(ws, n // 4)))
        for i, (_, per) in enumerate(tracks):
            if contig == "chrC" and i == 1:
                continue                                                       # (a track without this contig)
            an, y = [], r.randint(0, 500)
            while y < x:
                ln = r.randint(100, 1500 + 700 * i)
                an.append((y, y + ln))
                y += ln + r.randint(200, 4000)
            per[contig] = seg_array(an)
    return dict(segments=segments, annotations=tracks, workspace=workspace, isochores=None)
