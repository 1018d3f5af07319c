"""GPU: k_profile.  gat_list_profile against the model (tests/profile_model.py) on hand-made geometry, the argument errors,
gat_sample_profile_enrichment against the model applied to Problem.sample of the SAME problem, seed and sample range, and
scripts/gat-profile.py against the table built here from Problem.sample and the model.  Every comparison is exact: integers, or
the text of a table.  Every case runs at both staging limits and three runs of lists."""
import io
import itertools
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import profile_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
ANCHORS = ("default", "4")              # GAT_PROFILE_LDS_ANCHORS: a (track, group) of 5 anchors and more ends in global memory at 4
RUNS = ("default", "1", "3")            # GAT_PROFILE_SAMPLES_PER_BLOCK
KNOBS = list(itertools.product(ANCHORS, RUNS))
MODES = (M.BASES, M.MIDPOINTS)
TOP = 2 ** 32 - 1
ERR_ARG = -6


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_knobs(ctx, monkeypatch, anchors, run):
    for key, value in (("GAT_PROFILE_LDS_ANCHORS", anchors), ("GAT_PROFILE_SAMPLES_PER_BLOCK", run)):
        if value != "default":
            monkeypatch.setitem(ctx.options, key, value)
        else:
            monkeypatch.delitem(ctx.options, key, raising=False)


def seg_array(pairs):
    a = np.zeros(len(pairs), dtype=_lib.SEG)
    if len(pairs):
        a["start"], a["end"] = np.array(pairs, dtype=np.int64).T
    return a


def csr(entities):
    """entities[i][g] as lists of (start, end) -> (SEG array, offsets), entity-major"""
    flat = [x for e in entities for x in e]
    off = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64)
    return seg_array([p for x in flat for p in x]), off


def device_values(ctx, lists, anchors, w, H, mode):
    a, a_off = csr(lists)
    pos, minus, off = M.anchor_arrays(anchors)
    return ctx.list_profile(a, a_off, len(lists), pos, minus, off, len(anchors), len(anchors[0]), w, H, mode)


# ---- 1. gat_list_profile --------------------------------------------------------------------------------------------------------------
def spread(r, n, span):
    """n distinct anchors below span, ascending, plus before minus at one position; every fourth position carries both strands"""
    out = []
    for p in sorted(r.sample(range(span), n)):
        out.append((p, r.choice([+1, -1])))
    for k in range(0, len(out) - 1, 4):
        out[k + 1] = (out[k][0], -1)
        out[k] = (out[k][0], +1)
    return sorted(set(out), key=lambda x: (x[0], -x[1]))[:n]


def hand_geometry():
    """(name, lists[l][g], anchors[t][g], w, H): at most 3 groups, 3 tracks, 6 lists"""
    cases = []
    example_l = [[[(85, 112)]]]
    example_a = [[[(100, +1)]], [[(100, -1)]], [[(100, +1), (100, -1)]]]
    cases.append(("example", example_l, example_a, 10, 2))
    # list lengths 0, 1, 63, 64, 65, 130 (the lane stride and its tail); anchors per (track, group) 0, 1, 4, 5, 17 (the staging
    # limit and the block table); group 1: anchors, and lists without a segment; group 2: segments, and track 0 without an
    # anchor; track 2 is empty.  At B = 2, 64, 66 and 1024, the last with bins of one base
    r = random.Random(23)
    span = 2000
    lens_l = []
    for k, n in enumerate((0, 1, 63, 64, 65, 130)):
        g0 = M.random_normalized(r, n, span, 12)
        assert len(g0) == n
        lens_l.append([g0, M.random_normalized(r, 9, span, 30) if k % 2 else [], M.random_normalized(r, 20, span, 5)])
    a17 = spread(r, 17, span)
    assert len(a17) == 17
    lens_a = [[a17, [(700, -1)], []], [spread(r, 4, span), spread(r, 5, span), spread(r, 4, span)], [[], [], []]]
    for w, H in ((50, 1), (3, 32), (3, 33), (1, 512)):
        cases.append(("lengths-B%d" % (2 * H), lens_l, lens_a, w, H))
    # a segment over a whole window and more; windows of neighbouring anchors that overlap; plus and minus at one position
    over_l = [[[(0, 1000)]], [[(250, 300), (300, 340), (395, 400)]], [[(349, 350)]]]
    over_a = [[[(300, +1), (320, +1), (330, +1), (330, -1), (500, -1)]], [[(300, -1)]]]
    cases.append(("overlapping-windows", over_l, over_a, 10, 5))
    # a segment bookended with each window edge on each strand: (1000, +) has [900, 1100), (1000, -) has [901, 1101)
    book_l = [[[(890, 900), (1100, 1110)]], [[(900, 905), (1095, 1100)]], [[(895, 901), (1101, 1105)]], [[(901, 903), (1099, 1101)]]]
    book_a = [[[(1000, +1)]], [[(1000, -1)]]]
    cases.append(("bookended", book_l, book_a, 10, 10))
    # a at 0 and at 2^32 - 1 with R = 2^31, segments that reach 2^32 - 1.  With bins of 2^31 bases a track holds one anchor
    # (K_t * w < 2^32); with 1024 bins of 2^22, several
    far_l = [[[(0, TOP)], []], [[(5, 10), (2 ** 31 - 3, 2 ** 31 + 3), (TOP - 1, TOP)], [(TOP - 9, TOP)]], [[(0, 1)], [(2 ** 31, 2 ** 31 + 1)]]]
    for sigma, name in ((+1, "plus"), (-1, "minus")):
        cases.append(("far-%s" % name, far_l, [[[(0, sigma)], []], [[(TOP, sigma)], []], [[], [(2 ** 31, sigma)]]], 2 ** 31, 1))
    far_a = [[[(0, +1), (0, -1), (TOP, +1), (TOP, -1)], [(2 ** 31, -1)]], [[(1, -1), (TOP - 1, +1)], [(0, +1), (TOP, -1)]]]
    cases.append(("far-B1024", far_l, far_a, 2 ** 22, 512))
    return cases


def test_hand_geometry_is_what_it_says():
    by_name = {c[0]: c for c in hand_geometry()}
    for _, _, anchors, _, _ in by_name.values():        # ascending by position, plus before minus, none twice
        for keys in ([2 * a + (sigma < 0) for a, sigma in g] for t in anchors for g in t):
            assert all(x < y for x, y in zip(keys, keys[1:]))
    _, lists, anchors, w, H = by_name["example"]
    assert M.all_values(lists, anchors, w, H)[0].tolist() == [[5, 10, 10, 2], [1, 10, 10, 6], [6, 20, 20, 8]]
    assert M.all_values(lists, anchors, w, H, M.MIDPOINTS)[0].tolist() == [[0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 1, 0]]
    _, lists, anchors, w, H = by_name["bookended"]
    want = M.all_values(lists, anchors, w, H)
    assert want[0, 0].sum() == 0 and want[0, 1].tolist() == [1] + [0] * 19             # (1100 is the minus window's first base)
    assert want[1, 0].tolist() == [5] + [0] * 18 + [5] and want[2, 1].sum() == 0 and want[2, 0].tolist() == [1] + [0] * 19
    assert want[3, 1].tolist() == [2] + [0] * 18 + [2]
    _, lists, anchors, w, H = by_name["overlapping-windows"]
    assert M.all_values(lists, anchors, w, H)[0].tolist() == [[50] * 10, [10] * 10]       # every bin whole, once per anchor
    _, lists, anchors, w, H = by_name["far-plus"]
    assert M.all_values(lists, anchors, w, H)[0].tolist() == [[0, 2 ** 31], [2 ** 31, 0], [0, 0]]
    _, lists, anchors, w, H = by_name["lengths-B66"]
    assert [len(l[0]) for l in lists] == [0, 1, 63, 64, 65, 130] and [[len(g) for g in t] for t in anchors] == [[17, 1, 0], [4, 5, 4], [0, 0, 0]]
    assert any(a[k][0] == a[k + 1][0] for a in (anchors[0][0],) for k in range(16))     # plus and minus at one position


@pytest.mark.parametrize("mode", MODES, ids=["bases", "midpoints"])
@pytest.mark.parametrize("case", hand_geometry(), ids=lambda c: c[0])
def test_list_profile(ctx, monkeypatch, case, mode):
    """the model's values, whatever the staging limit and the run"""
    name, lists, anchors, w, H = case
    assert len(lists) <= 6 and len(anchors) <= 3 and all(len(l) <= 3 and all(M.is_normalized(x) for x in l) for l in lists)
    want = M.all_values(lists, anchors, w, H, mode)
    assert want.sum() > 0
    for k_anchors, run in KNOBS:
        set_knobs(ctx, monkeypatch, k_anchors, run)
        got = device_values(ctx, lists, anchors, w, H, mode)
        assert got.dtype == np.int64 and got.shape == want.shape == (len(lists), len(anchors), 2 * H)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, k_anchors, run, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ---- 2. the argument errors -----------------------------------------------------------------------------------------------------------
def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, off = seg_array([(85, 112), (130, 140)]), np.array([0, 2], dtype=np.int64)
    pos, minus, aoff = np.array([100, 100], dtype=np.uint32), np.array([0, 1], dtype=np.uint8), np.array([0, 2], dtype=np.int64)
    out = np.full((1, 1, 4), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, ps=pos, mi=minus, ao=aoff, t=1, g=1, w=10, h=2, mode=0, o=out):
        return L.gat_list_profile(c, p(lists), p(lo), n, p(ps), p(mi), p(ao), t, g, w, h, mode, p(o))

    def message(**bad):
        assert call(**bad) == ERR_ARG, bad
        return L.gat_last_error(ctx._h)

    assert call() == 0 and out[0, 0].tolist() == [6, 20, 20, 8]
    assert call(mode=1) == 0 and out[0, 0].tolist() == [0, 1, 1, 0]
    assert call() == 0
    keep = out.copy()
    for bad in (dict(c=None), dict(lo=None), dict(ao=None), dict(o=None), dict(lists=None), dict(ps=None), dict(mi=None), dict(n=-1),
                dict(t=-1), dict(g=-1), dict(lo=np.array([2, 0], dtype=np.int64)), dict(ao=np.array([2, 0], dtype=np.int64)),
                dict(w=0), dict(w=-5), dict(w=2 ** 31 + 1), dict(h=0), dict(h=-1), dict(h=513), dict(h=512, w=2 ** 22 + 1), dict(mode=2),
                dict(mode=-1)):
        assert call(**bad) == ERR_ARG, bad
    assert b"bin_size 0 outside" in message(w=0) and b"half_bins 513 outside" in message(h=513) and b"mode 2" in message(mode=2)
    assert b"more than 2^31" in message(h=512, w=2 ** 22 + 1)
    # the anchors of a (track, group): ascending, plus before minus, none twice, the strand 0 or 1 -- named by track and group
    a3 = np.array([7, 100, 100, 50, 60], dtype=np.uint32)
    o3 = np.array([0, 1, 1, 3, 3, 5, 5], dtype=np.int64)          # 2 tracks x 3 groups: (0,0) 1, (0,2) 2, (1,1) 2
    l3, lo3 = csr([[[(0, 4)], [(2, 3)], []]])
    out3 = np.full((1, 2, 4), -1, dtype=np.int64)
    three = dict(lists=l3, lo=lo3, ps=a3, ao=o3, t=2, g=3, o=out3)
    assert call(mi=np.array([0, 0, 1, 0, 1], dtype=np.uint8), **three) == 0
    assert b"anchor track 0, group 2 is out of order at anchor 1" in message(mi=np.array([0, 1, 0, 0, 1], dtype=np.uint8), **three)
    assert b"anchor track 0, group 2 repeats an anchor" in message(mi=np.array([0, 1, 1, 0, 1], dtype=np.uint8), **three)
    assert b"anchor track 1, group 1: anchor_minus 2" in message(mi=np.array([0, 0, 1, 0, 2], dtype=np.uint8), **three)
    down = dict(three, ps=np.array([7, 100, 100, 60, 50], dtype=np.uint32))
    assert b"anchor track 1, group 1 is out of order at anchor 1" in message(mi=np.array([0, 0, 1, 0, 0], dtype=np.uint8), **down)
    # the lists must be normalized, and the message names the list and the group
    for bad in ([(0, 4), (3, 8)], [(4, 8), (0, 4)], [(0, 4), (6, 6)]):
        bl, blo = csr([[[(0, 4)], bad, []]])
        assert b"segment list 0, group 1 is not normalized" in message(mi=np.array([0, 0, 1, 0, 1], dtype=np.uint8), **dict(three, lists=bl, lo=blo))
    # a value is a 32-bit word: K_t * bin_size < 2^32
    assert b"does not fit 32 bits" in message(w=2 ** 31, h=1, o=np.zeros((1, 1, 2), dtype=np.int64))
    assert call(w=2 ** 31, h=1, ps=pos[:1], mi=minus[:1], ao=np.array([0, 1], dtype=np.int64), o=np.zeros((1, 1, 2), dtype=np.int64)) == 0
    assert np.array_equal(out, keep) and out3.min() >= 0
    # nothing to do: nothing is written
    out[:] = -1
    assert call(n=0, lo=np.array([0], dtype=np.int64)) == 0 and call(t=0, ao=np.array([0], dtype=np.int64)) == 0 and out.min() == out.max() == -1


# ---- 3. gat_sample_profile_enrichment ---------------------------------------------------------------------------------------------------
SEED, SAMPLES, FEW, SPLIT = 77, 40, 7, 5
PROBLEMS = ("annotator-units", "shift-units", "brute-force-units", "annotator-genome-isochores") + CC.CIRCULAR_NAMES
BIN_SIZE, HALF_BINS = 25, 10


def anchors_for(flat, seed=5):
    """three tracks of anchors inside the workspace of every contig: 17 and more a contig on both strands (windows that overlap
    on the short contigs), three a contig, and six on the longest contig alone"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = [[], [], []]
    for c in range(len(ext)):
        span = max(60, int(ext[c]))
        tracks[0].append(spread(r, min(19, span // 3), span))
        tracks[1].append([(span * (k + 1) // 4, (+1, -1, +1)[k]) for k in range(3)])
        tracks[2].append([(span * (k + 1) // 8, (-1) ** k) for k in range(6)] if c == int(np.argmax(ext)) else [])
    return tracks


def observed_for(values):
    """an obs per (track, bin) that meets the null where it can: the value of sample 1, that value + 1 in every third bin, 0 in
    every fifth"""
    obs = values[1].copy()
    obs[:, ::3] += 1
    obs[:, ::5] = 0
    return obs


@pytest.fixture(scope="module")
def sampled(ctx):
    """per problem: the flat problem, its anchors, Problem.sample of (SEED, 0, SAMPLES) -- drawn once -- and per mode the
    model's values [samples][tracks][bins] of those lists"""
    cache = {}

    def get(name, mode=None):
        if name not in cache:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            try:
                seg, off = P.sample(SEED, 0, SAMPLES)
                n_contigs = P.n_contigs
            finally:
                P.close()
            cache[name] = dict(flat=flat, anchors=anchors_for(flat), seg=seg, off=off, n_contigs=n_contigs, values={})
        e = cache[name]
        if mode is not None and mode not in e["values"]:
            e["values"][mode] = M.from_sample(e["seg"], e["off"], e["n_contigs"], e["anchors"], BIN_SIZE, HALF_BINS, mode)
        return e
    return get


def same_words(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


@pytest.mark.parametrize("mode", MODES, ids=["bases", "midpoints"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_samplers(ctx, sampled, monkeypatch, name, mode):
    e = sampled(name, mode)
    values = e["values"][mode]
    assert all(M.is_normalized(e["seg"][e["off"][l]:e["off"][l + 1]]) for l in range(len(e["off"]) - 1))
    assert values.shape == (SAMPLES, 3, 2 * HALF_BINS)
    obs = observed_for(values)
    want = M.words(values, obs)
    pos, minus, off = M.anchor_arrays(e["anchors"])
    P = _lib.Problem(ctx, e["flat"])
    try:
        for k_anchors, run in KNOBS:
            set_knobs(ctx, monkeypatch, k_anchors, run)
            what = (name, mode, k_anchors, run)
            got = P.sample_profile_enrichment(SEED, 0, SAMPLES, pos, minus, off, 3, BIN_SIZE, HALF_BINS, mode, obs)
            same_words(got, want, what)
            few = P.sample_profile_enrichment(SEED, 0, FEW, pos, minus, off, 3, BIN_SIZE, HALF_BINS, mode, obs)
            same_words(few, M.words(values[:FEW], obs), what + ("[0, 7)",))
            # a range that does not start at 0, and split additivity: [0, 40) is [0, 5) and [5, 40)
            a = P.sample_profile_enrichment(SEED, 0, SPLIT, pos, minus, off, 3, BIN_SIZE, HALF_BINS, mode, obs)
            b = P.sample_profile_enrichment(SEED, SPLIT, SAMPLES, pos, minus, off, 3, BIN_SIZE, HALF_BINS, mode, obs)
            same_words(b, M.words(values[SPLIT:], obs), what + ("[5, 40)",))
            assert np.array_equal(a + b, got)
        # not vacuous: every track has a bin that a sample reaches, and some observed value lies inside the null
        n_pos, n_less, n_eq = got[..., 0], got[..., 3], got[..., 4]
        assert (n_pos > 0).any(axis=1).all() and ((n_less > 0) & (n_less < SAMPLES)).any()
        assert (n_less + n_eq <= SAMPLES).all() and got[..., 1].sum() == values.sum()
    finally:
        P.close()


def test_many_batches(ctx, sampled, monkeypatch):
    """a scratch budget of a few samples: the range goes through in several batches, the words are those of one"""
    e = sampled("annotator-genome-isochores", M.BASES)
    values = e["values"][M.BASES]
    obs = observed_for(values)
    pos, minus, off = M.anchor_arrays(e["anchors"])
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, e["flat"])
    try:
        got = P.sample_profile_enrichment(SEED, 0, SAMPLES, pos, minus, off, 3, BIN_SIZE, HALF_BINS, M.BASES, obs)
        assert P.last_stats["n_batches"] >= 2, P.last_stats["n_batches"]
    finally:
        P.close()
    same_words(got, M.words(values, obs), "batches")


def test_sample_arguments(ctx, sampled):
    L = _lib.lib()
    p = _lib._p
    e = sampled("annotator-units", M.BASES)
    values = e["values"][M.BASES]
    pos, minus, off = M.anchor_arrays(e["anchors"])
    B = 2 * HALF_BINS
    obs = observed_for(values)
    P = _lib.Problem(ctx, e["flat"])
    try:
        C_ = P.n_contigs
        out = np.full((3, B, 5), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, ps=pos, mi=minus, ao=off, t=3, w=BIN_SIZE, h=HALF_BINS, mode=0, ob=obs, o=out):
            return L.gat_sample_profile_enrichment(c, prob, SEED, begin, end, p(ps), p(mi), p(ao), t, w, h, mode, p(ob), p(o), None)

        def message(**bad):
            assert call(**bad) == ERR_ARG, bad
            return L.gat_last_error(ctx._h)

        assert call() == 0
        same_words(out, M.words(values[:2], obs), "two samples")
        keep = out.copy()
        down = off.copy()
        down[1] = down[2] + 1
        negative = obs.copy()
        negative[1, 3] = -1
        for bad in (dict(c=None), dict(prob=None), dict(ao=None), dict(ob=None), dict(o=None), dict(ps=None), dict(mi=None),
                    dict(begin=3, end=2), dict(t=-1), dict(ao=down), dict(w=0), dict(w=2 ** 31 + 1), dict(h=0), dict(h=513),
                    dict(h=512, w=2 ** 22 + 1), dict(mode=2), dict(ob=negative)):
            assert call(**bad) == ERR_ARG, bad
        assert b"bin_size 0 outside" in message(w=0) and b"negative" in message(ob=negative) and b"half_bins 0" in message(h=0)
        # sumsq must fit: (K_t * bin_size)^2 * samples < 2^64.  Track 0 holds K anchors: the bin size at which 2 samples pass
        K = int(off[C_] - off[0])
        w_big = (2 ** 32 - 1) // K
        assert b"sumsq" in message(w=w_big, h=1) and call(w=w_big, h=1, end=1) == 0
        assert b"does not fit 32 bits" in message(w=w_big + 1, h=1, end=1)
        # anchors out of order are named: track 1, the problem's contig 2
        at = int(off[1 * C_ + 2])
        assert off[1 * C_ + 2 + 1] - at >= 2
        bad_pos = pos.copy()
        bad_pos[at + 1] = bad_pos[at] - 1
        assert b"anchor track 1, group 2 is out of order at anchor 1" in message(ps=bad_pos)
        bad_pos[at + 1], bad_minus = bad_pos[at], minus.copy()
        bad_minus[at + 1] = bad_minus[at]
        assert b"anchor track 1, group 2 repeats an anchor" in message(ps=bad_pos, mi=bad_minus)
        bad_minus = minus.copy()
        bad_minus[at] = 3
        assert b"anchor track 1, group 2: anchor_minus 3" in message(mi=bad_minus)
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == 0           # an empty range writes zeros
        out[:] = -1
        assert call(t=0, ao=np.array([0], dtype=np.int64)) == 0 and out.min() == out.max() == -1       # no track: nothing is written
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], SEED, 0, 2, dev)
            assert b"in flight" in message()
            P.wait()
        finally:
            ctx.free(dev)
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()


def test_unsorted_sampler_is_refused(ctx):
    """SamplerSegments without isochore keys leaves lists that are neither sorted nor disjoint: refused, and the message says so"""
    flat = CC.genome_problem(CC.SEGMENTS, False)
    pos, minus, off = M.anchor_arrays(anchors_for(flat))
    P = _lib.Problem(ctx, flat)
    try:
        seg, soff = P.sample(SEED, 0, 4)
        assert not all(M.is_normalized(seg[soff[l]:soff[l + 1]]) for l in range(len(soff) - 1))
        with pytest.raises(ValueError, match="not normalized .SamplerSegments without isochore keys"):
            P.sample_profile_enrichment(SEED, 0, 4, pos, minus, off, 3, BIN_SIZE, HALF_BINS, 0, np.zeros((3, 2 * HALF_BINS), dtype=np.int64))
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        pos, minus, off = M.anchor_arrays([[[(1, +1)] for _ in range(P.n_contigs)]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_profile_enrichment(1, 0, 1, pos, minus, off, 1, 10, 1, 0, np.zeros((1, 2), dtype=np.int64))
    finally:
        P.close()


# ---- 4. the script --------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES, CLI_BIN, CLI_HALF = 11, 30, 50, 6     # (bins narrow enough that not every sample reaches every bin)


def anchor_file(path):
    """a small stranded anchor file over the contigs of tests/golden/cli: two named tracks, alternative transcripts that share a
    start site, an anchor just outside the workspace, and a contig the workspace lacks"""
    r = random.Random(2)
    lines = []
    for contig, top in (("chrA", 388000), ("chrB", 238000), ("chrC", 78000), ("chrD", 38000)):
        for k in range(8):
            s = r.randrange(12000, top - 3000)
            lines.append("%s\t%d\t%d\t%s\t0\t%s" % (contig, s, s + r.randrange(1, 2500), "tss" if k % 4 else "other", "+-"[k % 2]))
            if k == 6:
                lines.append("%s\t%d\t%d\ttss\t0\t+" % (contig, s, s + 7))          # a second transcript from the same start site
    lines.append("chrA\t11990\t11995\ttss\t0\t+")
    lines.append("chrNowhere\t5\t9\ttss\t0\t-")
    path.write_text("\n".join(lines) + "\n")
    return str(path)


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--order=track"],
                                   ["--with-segment-tracks", "--qvalue-method=holm", "--profile-of=midpoints", "--anchor-point=three-prime"],
                                   ["--ignore-strand", "--annotations-label=all", "--order=annotation"], ["--sampler=circular"]],
                         ids=["isochores", "tracks-midpoints", "pooled", "circular"])
def test_script(ctx, tmp_path, extra):
    """the printed table is the one built here: Problem.sample of the same inputs and seeds, the model's values and words"""
    from gat_amd import profile, problem
    from test_profile_host import script
    mod = script()
    bed = anchor_file(tmp_path / "anchors.bed")
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--anchors=%s" % bed,
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--bin-size=%d" % CLI_BIN, "--half-bins=%d" % CLI_HALF, "--verbose=0"] + extra
    assert mod.main(["gat-profile.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    opts, _ = mod.buildParser().parse_args(argv)
    mode = profile.PROFILES_OF.index(opts.profile_of)
    segments, annotations, workspace = profile.build_inputs(opts)
    read = profile.read_anchors(opts.annotation_files, opts.anchor_point, opts.ignore_strand, opts.annotations_label)
    assert list(read) == (["merged"] if opts.annotations_label else ["other", "tss"])
    results = []
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, wa = profile.flatten(segments[track], workspace, profile.make_sampler(opts))
        contigs = list(flat["contig_names"])
        assert "chrNowhere" not in contigs
        csegs = problem.from_isochores(sa)
        anchors = [[[(int(a), -1 if m else +1) for a, m in zip(*read[t][c])] if c in read[t] else [] for c in contigs] for t in read]
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        obs = M.all_values([[csegs.get(c, []) for c in contigs]], anchors, CLI_BIN, CLI_HALF, mode)[0]
        words = M.words(M.from_sample(seg, off, len(contigs), anchors, CLI_BIN, CLI_HALF, mode), obs)
        results.extend(profile.rows(track, list(read), [sum(len(g) for g in t) for t in anchors], CLI_BIN, CLI_HALF, obs, words, CLI_SAMPLES))
    profile.set_qvalues(results, opts.qvalue_method)
    sink = io.StringIO()
    profile.write_results(sink, results, opts.output_order)
    got = "".join(l for l in open(str(tmp_path / "got.tsv")) if not l.startswith("#"))
    assert got == sink.getvalue()
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    assert len(rows) == len(list(segments.tracks)) * len(read) * 2 * CLI_HALF and all(len(r) == 14 for r in rows)
    assert any(int(r[5]) > 0 and float(r[6]) > 0 for r in rows) and any(0 < int(r[12]) < CLI_SAMPLES for r in rows)
    # the anchor outside the workspace is kept, the shared start sites are one anchor, the contig the workspace lacks is dropped
    if not opts.annotations_label and not opts.ignore_strand and opts.anchor_point == "five-prime":
        assert sorted(set(int(r[13]) for r in rows)) == [8, 25]
