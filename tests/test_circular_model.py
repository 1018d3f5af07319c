"""CPU: tests/circular_model.py against a base-by-base brute force, the contract's invariants, and the sampler's place in
the package -- the class and the command line."""
import random

import pytest

import circular_model as M
import gat_amd


def _tiny_unit(r):
    """a unit of Wsum <= 60 and 1-5 workspace pieces (touching ones among them), segments in and around them."""
    ws, x = [], r.randint(0, 5)
    left = r.randint(1, 60)
    for k in range(r.randint(1, 5)):
        if left == 0:
            break
        ln = r.randint(1, left)
        ws.append((x, x + ln))
        left -= ln
        x += ln + r.choice((0, 0, 1, 3, 7))             # 0: a touching piece, kept apart
    hi = ws[-1][1] + 4
    pts = sorted(r.sample(range(0, hi + 1), min(hi + 1, 2 * r.randint(1, 6))))
    segs = [(pts[2 * i], pts[2 * i + 1]) for i in range(len(pts) // 2)]
    if r.random() < 0.15:                               # one piece filled by one segment, all of W covered
        segs = [(ws[0][0], ws[-1][1])]
    return segs, ws


def _brute(segs, ws, r):
    """rotate the set of linear base indices, then read the genome base by base: a piece ends where the workspace piece
    ends, where the next base comes from another working interval, and where the source wraps from Wsum - 1 to 0."""
    genome = [x for s, e in ws for x in range(s, e)]            # linear index -> genome position
    first = {s for s, _ in ws}
    wsum = len(genome)
    covered = {x for s, e in segs for x in range(s, e)}
    owner, run, prev = [None] * wsum, -1, False
    for p in range(wsum):                                       # working interval of every linear base
        here = genome[p] in covered
        if here and not prev:
            run += 1
        owner[p] = run if here else None
        prev = here
    out = []
    for p in range(wsum):
        src = (p - r) % wsum
        if owner[src] is None:
            continue
        g = genome[p]
        cont = (out and out[-1][1] == g and g not in first and src != 0 and owner[(p - 1 - r) % wsum] == owner[src])
        if cont:
            out[-1][1] = g + 1
        else:
            out.append([g, g + 1])
    return [tuple(x) for x in out]


UNITS = [_tiny_unit(random.Random(1000 + i)) for i in range(120)]


def test_model_vs_brute_force():
    """every r of 120 random tiny units"""
    seen_wrap = seen_touch = 0
    for segs, ws in UNITS:
        iv = M.linear_intervals(segs, ws)
        wsum = M.workspace_sum(ws)
        for r in range(wsum):
            got = M.rotate(iv, ws, r)
            assert got == _brute(segs, ws, r), (segs, ws, r)
            seen_wrap += any(a + r < wsum < b + r for a, b in iv)
            seen_touch += any(x[1] == y[0] for x, y in zip(got, got[1:]))
    assert seen_wrap > 100 and seen_touch > 100


def test_invariants():
    """every piece inside W; the bases kept; rotating back by r gives the working list; at most n + |W| pieces"""
    for segs, ws in UNITS:
        iv = M.linear_intervals(segs, ws)
        wsum = M.workspace_sum(ws)
        assert all(a < b for a, b in iv) and all(x[1] < y[0] for x, y in zip(iv, iv[1:]))
        bases = sum(b - a for a, b in iv)
        for r in range(wsum):
            got = M.rotate(iv, ws, r)
            assert all(any(s <= a and b <= e for s, e in ws) for a, b in got)
            assert all(a < b for a, b in got) and all(x[1] <= y[0] for x, y in zip(got, got[1:]))
            assert sum(b - a for a, b in got) == bases
            assert len(got) <= len(iv) + len(ws)
            # back: the sample's linear bases moved by -r are the working list's
            back = sorted((x - r) % wsum for a, b in M.linear_intervals(got, ws) for x in range(a, b))
            assert back == [x for a, b in iv for x in range(a, b)]
        if iv:
            assert M.rotate(iv, ws, 0) == [p for a, b in iv for p in M.to_genome(ws, a, b)]


def test_hand_made_units():
    # a segment bridging a workspace gap is one interval; one hanging over the workspace's edge is cut
    assert M.linear_intervals([(5, 25), (38, 50)], [(0, 10), (20, 40)]) == [(5, 15), (28, 30)]
    # touching workspace pieces stay two: the observed list (r == 0) is cut at their border
    assert M.rotate(M.linear_intervals([(5, 15)], [(0, 10), (10, 20)]), [(0, 10), (10, 20)], 0) == [(5, 10), (10, 15)]
    # one piece filled by one segment: two touching pieces for r > 0, the piece itself for r == 0
    assert M.rotate([(0, 10)], [(100, 110)], 3) == [(100, 103), (103, 110)]
    assert M.rotate([(0, 10)], [(100, 110)], 0) == [(100, 110)]
    # an interval ending exactly at Wsum is not cut; one starting exactly at the wrap lands at the workspace's start
    assert M.rotate([(2, 5)], [(0, 4), (6, 12)], 5) == [(9, 12)]
    assert M.rotate([(2, 5)], [(0, 4), (6, 12)], 8) == [(0, 3)]
    assert M.rotate([(2, 5)], [(0, 4), (6, 12)], 6) == [(0, 1), (10, 12)]


def test_no_draw_without_intervals():
    class NoDraw(object):
        def randint(self, lo, hi):
            raise AssertionError("drew")
    assert M.sample(NoDraw(), [(50, 60)], [(0, 10)]) == []
    assert M.sample(NoDraw(), [], [(0, 10)]) == []
    assert M.sample(NoDraw(), [(0, 5)], []) == []


def test_sampler_class_and_parser():
    s = gat_amd.SamplerCircular()
    assert s.kind == 6 and isinstance(s, gat_amd.Sampler)
    assert gat_amd.engine.SamplerCircular is gat_amd.SamplerCircular
    assert gat_amd.TOOL_SAMPLERS == gat_amd.CLI_SAMPLERS + ("circular",)
    for arg in (["-m", "circular"], ["--sampler=circular"]):
        opts, _ = gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS).parse_args(arg)
        assert opts.sampler == "circular"
    with pytest.raises(SystemExit):                         # (a bare buildParser() stays as it was)
        gat_amd.buildParser().parse_args(["-m", "circular"])
