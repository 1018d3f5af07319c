"""CPU: tests/universe_model.py -- the draw proved uniform by enumerating every draw sequence, k against a base-by-base brute
force, the complement switch, and the sampler's place on the command line."""
import itertools
import math
import random

import pytest

import gat_amd
import universe_model as M


def test_floyd_is_exactly_uniform():
    """every m <= 7 and every c: the m! / (m - c)! draw sequences (t_j in range(j + 1) for j = m - c .. m - 1) reach each of the
    C(m, c) subsets exactly c! times.  No statistics: a count."""
    for m in range(0, 8):
        for c in range(0, m + 1):
            ranges = [range(j + 1) for j in range(m - c, m)]
            seen = {}
            n_seq = 0
            for seq in itertools.product(*ranges):
                it = iter(seq)
                marked = M.floyd(lambda j: next(it), m, c)
                assert len(marked) == c and all(0 <= h < m for h in marked)
                key = tuple(sorted(marked))
                seen[key] = seen.get(key, 0) + 1
                n_seq += 1
            assert n_seq == math.factorial(m) // math.factorial(m - c)
            assert len(seen) == math.comb(m, c), (m, c)
            assert set(seen.values()) == {math.factorial(c)}, (m, c)


def _brute_hits(segs, ws):
    covered = {x for s, e in segs for x in range(s, e)}
    return sum(1 for s, e in ws if any(x in covered for x in range(s, e)))


def _tiny(r):
    """1-8 workspace pieces, touching ones among them; segments inside, across borders, at borders and outside."""
    ws, x = [], r.randint(0, 6)
    for _ in range(r.randint(1, 8)):
        ln = r.randint(1, 9)
        ws.append((x, x + ln))
        x += ln + r.choice((0, 0, 1, 2, 6))
    hi = ws[-1][1] + 8
    pts = sorted(r.sample(range(0, hi + 1), min(hi + 1, 2 * r.randint(1, 7))))
    segs = [(pts[2 * i], pts[2 * i + 1]) for i in range(len(pts) // 2)]
    if r.random() < 0.2:                                   # a segment that ends / begins exactly at a piece's border
        j = r.randrange(len(ws))
        segs = [(ws[j][1], ws[j][1] + 2)] if r.random() < 0.5 else [(max(0, ws[j][0] - 2), ws[j][0])]
        segs = [s for s in segs if s[0] < s[1]]
    return segs, ws


def test_hits_vs_brute_force():
    spanning = outside = touching = 0
    for i in range(600):
        segs, ws = _tiny(random.Random(7000 + i))
        k = M.hits(segs, ws)
        assert k == _brute_hits(segs, ws), (segs, ws)
        spanning += any(sum(1 for a, b in ws if a < e and s < b) > 1 for s, e in segs)
        outside += any(all(not (a < e and s < b) for a, b in ws) for s, e in segs)
        touching += any(e == a or s == b for s, e in segs for a, b in ws)
    assert spanning > 100 and outside > 100 and touching > 100


def test_hand_made_hits():
    ws = [(0, 10), (10, 20), (30, 40)]
    assert M.hits([(5, 15)], ws) == 2                      # a segment over two (touching) pieces hits two
    assert M.hits([(20, 30)], ws) == 0                     # in the gap, touching both neighbours: none
    assert M.hits([(50, 60)], ws) == 0
    assert M.hits([(1, 2), (3, 4), (5, 6)], ws) == 1       # three segments in one piece: one hit
    assert M.hits([(9, 31)], ws) == 3
    assert M.hits([], ws) == 0 and M.hits([(0, 5)], []) == 0


def test_complement_switch():
    assert M.smaller_side(3, 6) == (3, False)              # 2k == m: the marked side
    assert M.smaller_side(4, 7) == (3, True)               # 2k == m + 1: the unmarked side
    assert M.smaller_side(3, 7) == (3, False)
    assert M.smaller_side(0, 5) == (0, False) and M.smaller_side(5, 5) == (0, True) and M.smaller_side(1, 1) == (0, True)

    class Counting(object):
        def __init__(self, r):
            self.r, self.calls = r, []

        def randint(self, lo, hi):
            self.calls.append((lo, hi))
            return self.r.randrange(lo, hi)
    for k, m in ((3, 6), (4, 7), (3, 7), (6, 7), (1, 7)):
        rng = Counting(random.Random(k * 100 + m))
        got = M.choose(rng, k, m)
        c = min(k, m - k)
        assert len(got) == k and got == sorted(set(got)) and all(0 <= h < m for h in got)
        assert rng.calls == [(0, j + 1) for j in range(m - c, m)]


def test_nothing_drawn_at_the_ends():
    class NoDraw(object):
        def randint(self, lo, hi):
            raise AssertionError("drew")
    ws = [(0, 5), (7, 9), (9, 12)]
    assert M.sample(NoDraw(), [(20, 30)], ws) == []                         # k == 0
    assert M.sample(NoDraw(), [(0, 12)], ws) == ws                          # k == m
    assert M.sample(NoDraw(), [(3, 4)], [(0, 5)]) == [(0, 5)]               # m == 1
    assert M.sample(NoDraw(), [(3, 4)], []) == [] and M.sample(NoDraw(), [], ws) == []


def test_sample_is_k_whole_pieces():
    r = random.Random(5)
    for i in range(200):
        segs, ws = _tiny(random.Random(9000 + i))
        st = {}

        class R(object):
            def randint(self, lo, hi):
                return r.randrange(lo, hi)
        got = M.sample(R(), segs, ws, st)
        assert len(got) == st["k"] == M.hits(segs, ws) and got == sorted(got) and set(got) <= set(ws) and len(set(got)) == len(got)


def test_sampler_class_and_parser():
    s = gat_amd.SamplerUniverse()
    assert s.kind == 7 and isinstance(s, gat_amd.Sampler)
    assert gat_amd.engine.SamplerUniverse is gat_amd.SamplerUniverse
    assert gat_amd.UNIVERSE_SAMPLERS == ("universe",)
    assert gat_amd.TOOL_SAMPLERS == gat_amd.CLI_SAMPLERS + ("circular",)          # (as it was)
    for arg in (["-m", "universe"], ["--sampler=universe"]):
        opts, _ = gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS + gat_amd.UNIVERSE_SAMPLERS).parse_args(arg)
        assert opts.sampler == "universe"
    with pytest.raises(SystemExit):
        gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS).parse_args(["--sampler=universe"])
