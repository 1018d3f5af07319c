"""GPU: k_signal.  gat_list_signal against the model (tests/signal_model.py) on the hand cases and on lists around the
lane-stride and staging edges, against the kernels that already count bases and hits, gat_sample_signal against the model
applied to Problem.sample of the SAME problem, seed and sample range, and scripts/gat-signal.py against the table built here
from Problem.sample, the model and engine.AnnotatorResult.  Every comparison is exact: integers, or the text of a table."""
import io
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import signal_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
LDS = ("default", "8")                  # GAT_SIGNAL_LDS_PIECES: lists of 9 pieces and more end in global memory at 8
ERR_ARG = -6                            # GAT_ERR_ARG
INT32_MIN = -2 ** 31
Q_MAX = M.Q_MAX


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(params=LDS)
def lds(request, ctx, monkeypatch):
    if request.param != "default":
        monkeypatch.setitem(ctx.options, "GAT_SIGNAL_LDS_PIECES", request.param)
    return request.param


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


def track_csr(tracks):
    """tracks[t][g] = (pieces, values) -> (SEG array, int32 values, offsets), track-major"""
    pieces, off = csr([[g[0] for g in t] for t in tracks])
    values = np.array([v for t in tracks for g in t for v in g[1]], dtype=np.int64)
    assert len(values) == len(pieces) and (len(values) == 0 or np.abs(values).max() <= Q_MAX)
    return pieces, values.astype(np.int32), off


def device_words(ctx, lists, tracks):
    """lists[l][g] and tracks[t][g] = (pieces, values) -> int64 [n_lists, n_tracks, 4] from gat_list_signal"""
    n_groups = len(lists[0]) if lists else len(tracks[0])
    a, a_off = csr(lists)
    p, v, p_off = track_csr(tracks)
    return _lib.list_signal(ctx, a, a_off, len(lists), p, v, p_off, len(tracks), n_groups)


def check(ctx, lists, tracks, what=""):
    got = device_words(ctx, lists, tracks)
    want = M.all_words(lists, tracks)
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    return got


# ---- 1. gat_list_signal -------------------------------------------------------------------------------------------------------------
def test_hand_cases(ctx, lds):
    """every hand case on its own (the long pieces with the largest values allow no list that is not normalized beside them),
    then the segments of every small case against the pieces of every small case, one group"""
    sums = []
    for name, segs, pieces, values, want in M.HAND:
        got = device_words(ctx, [[segs]], [[(pieces, values)]])
        assert got[0, 0].tolist() == want, name
        sums.append(want[3])
    assert min(sums) < 0 and max(abs(s) for s in sums) > 2 ** 32
    small = [h for h in M.HAND if not h[3] or max(abs(v) for v in h[3]) < 100]
    assert len(small) >= len(M.HAND) - 2
    got = check(ctx, [[h[1]] for h in small], [[(h[2], h[3])] for h in small], "hand")
    for i, h in enumerate(small):
        assert got[i, i].tolist() == h[4], h[0]


T_SIZES = (0, 1, 2, 8, 9, 63, 64, 65, 129)
Q_SIZES = (0, 1, 63, 64, 65, 129)


def probes(pieces, k):
    """every piece itself, and the k bases to its left and to its right"""
    return [(a, b) for a, b in pieces] + [(a - k, a) for a, _ in pieces if a >= k] + [(b, b + k) for _, b in pieces]


def test_list_sizes(ctx, lds):
    """piece lists around the staging limit and its blocks (8, 9, 64, 65 at a limit of 8), segment lists around one and two
    rounds of 64 lanes: every pair, in one launch; the values of one track are +-(2^31 - 1)"""
    r = random.Random(7)
    tracks = [[M.random_pieces(r, k, 3000)] for k in T_SIZES]
    assert [len(t[0][0]) for t in tracks] == list(T_SIZES)
    big = M.random_pieces(r, 65, 3000)
    tracks.append([(big[0], [r.choice([-Q_MAX, Q_MAX]) for _ in big[0]])])
    top = max(t[0][0][-1][1] for t in tracks if t[0][0])
    lists = [[M.random_segments(r, n, top + 200)] for n in Q_SIZES]
    for k in (1, 3):
        for t in (tracks[T_SIZES.index(65)], tracks[T_SIZES.index(129)], tracks[-1]):
            lists.append([probes(t[0][0], k)])
    got = check(ctx, lists, tracks, "sizes")
    assert got[:, 1:, 2].sum() > 0 and (got[:, :, 2] < got[:, :, 0]).any() and (got[:, 0, 1:] == 0).all()
    assert (got[:, :, 0] == got[:, :1, 0]).all()                              # n is the same for every track
    assert got[:, :, 3].min() < 0 and np.abs(got[:, -1, 3]).max() > 2 ** 32


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("n_tracks", [1, 2, 5])
def test_tracks_and_groups(ctx, lds, n_tracks, n_groups):
    """the sums over the groups: seven segment lists, 1 / 2 / 5 tracks, 1 / 3 groups; with three groups one track is empty on
    one group and one list on another"""
    r = random.Random(100 * n_tracks + n_groups)
    tracks = [[M.random_pieces(r, r.choice([1, 3, 20, 70]), 2000) for _ in range(n_groups)] for _ in range(n_tracks)]
    lists = [[M.random_segments(r, r.choice([1, 5, 70]), 2500) for _ in range(n_groups)] for _ in range(7)]
    if n_groups > 1:
        tracks[n_tracks - 1][n_groups - 1] = ([], [])
        lists[2][0] = []
    got = check(ctx, lists, tracks, "groups")
    assert got[:, :, 0].sum() > 0 and got[:, :, 1].sum() > 0


def test_staging_limit_changes_no_result(ctx, monkeypatch):
    r = random.Random(3)
    tracks = [[M.random_pieces(r, k, 20000)] for k in (1, 64, 65, 200, 1000)]
    lists = [[M.random_segments(r, 150, 22000, max_len=400)] for _ in range(5)] + [[probes(tracks[4][0][0], 2)]]
    want = check(ctx, lists, tracks)
    for limit in ("1", "7", "200", "2048", "100000000"):
        monkeypatch.setitem(ctx.options, "GAT_SIGNAL_LDS_PIECES", limit)
        assert np.array_equal(device_words(ctx, lists, tracks), want), limit


def test_against_the_kernels_that_count_bases_and_hits(ctx, lds):
    """normalized lists: `covered` is the nucleotide overlap of the list with the pieces (gat_count_lists), `hit` the diagonal of
    gat_list_pair_hits on the pieces as a track, and with every value 1 the sum is `covered`"""
    r = random.Random(21)
    n_groups, n_tracks, n_lists = 3, 4, 6
    tracks = [[M.random_pieces(r, r.choice([2, 30, 90]), 4000, max_len=60, lo=1, hi=1) for _ in range(n_groups)] for _ in range(n_tracks)]
    lists = [[M.random_normalized(r, r.choice([1, 40, 100]), 4500) for _ in range(n_groups)] for _ in range(n_lists)]
    got = check(ctx, lists, tracks, "ones")
    assert np.array_equal(got[:, :, 3], got[:, :, 1]) and got[:, :, 1].sum() > 0 and (got[:, :, 2] < got[:, :, 0]).any()
    a, a_off = csr(lists)
    p, _, p_off = track_csr(tracks)
    overlap = ctx.count_lists(["nucleotide-overlap"], a, a_off, n_lists, p, p_off, n_tracks, [1] * n_groups, n_groups)[0]
    assert np.array_equal(got[:, :, 1], overlap.T)
    pairs = ctx.list_pair_hits(a, a_off, n_lists, p, p_off, n_tracks, n_groups)
    diagonal = [t * n_tracks - t * (t - 1) // 2 for t in range(n_tracks)]
    assert np.array_equal(got[:, :, 2], pairs[:, diagonal])


LONG_PIECE = 2 ** 31 + 2 ** 20


def overflow_track():
    """one track over two groups whose sum_g M passes 2^63: on each group one piece of a little over 2^31 bases with |q| =
    2^31 - 1.  (Two pieces of exactly 2^31 bases give 2^63 - 2^32, which every sum of a normalized list stays within: the
    pieces have to be longer than that to pass the bound.)"""
    assert 2 * Q_MAX * 2 ** 31 < 2 ** 63 <= 2 * Q_MAX * LONG_PIECE and Q_MAX * LONG_PIECE < 2 ** 63
    return [[([(0, LONG_PIECE)], [Q_MAX]), ([(5, LONG_PIECE + 5)], [-Q_MAX])]]


def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, pieces = seg_array([(1, 5), (30, 40)]), seg_array([(0, 4), (4, 8), (20, 32)])
    vals = np.array([3, -2, 10], dtype=np.int32)
    off, poff = np.array([0, 2], dtype=np.int64), np.array([0, 3], dtype=np.int64)
    out = np.full((1, 1, 4), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, a=pieces, v=vals, ao=poff, t=1, g=1, o=out):
        return L.gat_list_signal(c, p(lists), p(lo), n, p(a), p(v), p(ao), t, g, p(o))

    assert call() == 0 and out[0, 0].tolist() == M.words([(1, 5), (30, 40)], [(0, 4), (4, 8), (20, 32)], [3, -2, 10]) == [2, 6, 2, 27]
    keep = out.copy()
    out[:] = -1
    down = np.array([2, 0], dtype=np.int64)
    for bad in (dict(c=None), dict(lo=None), dict(ao=None), dict(o=None), dict(lists=None), dict(a=None), dict(v=None), dict(n=-1), dict(t=-1),
                dict(g=-1), dict(lo=down), dict(ao=np.array([3, 0], dtype=np.int64)), dict(v=np.array([3, INT32_MIN, 10], dtype=np.int32))):
        assert call(**bad) == ERR_ARG, bad
        assert out.min() == out.max() == -1, bad
    assert b"INT32_MIN" in L.gat_last_error(ctx._h) and b"signal track 0, group 0" in L.gat_last_error(ctx._h)
    # the tracks must be normalized; the segment lists need not be
    for bad in (seg_array([(0, 4), (3, 8), (20, 22)]), seg_array([(4, 8), (0, 4), (20, 22)]), seg_array([(0, 4), (6, 6), (20, 22)])):
        assert call(a=bad) == ERR_ARG and b"annotation track 0, group 0 is not normalized" in L.gat_last_error(ctx._h)
        assert out.min() == out.max() == -1
        assert call(lists=bad, lo=poff) == 0 and out.min() >= 0
        out[:] = -1
    # ... and the message names the track and the group: track 1 of 2, group 2 of 3
    a6, o6 = csr([[[(0, 4)], [], [(5, 6)]], [[(1, 2)], [(3, 4)], [(9, 12), (11, 13)]]])
    l3, lo3 = csr([[[(0, 4)], [(2, 3)], []]])
    out2 = np.full((1, 2, 4), -1, dtype=np.int64)
    assert call(lists=l3, lo=lo3, a=a6, v=np.ones(6, dtype=np.int32), ao=o6, t=2, g=3, o=out2) == ERR_ARG
    assert b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h)
    assert out2.min() == -1
    # nothing to compare: nothing written
    out[:] = -1
    assert call(n=0, lo=np.array([0], dtype=np.int64)) == 0 and call(t=0, ao=np.array([0], dtype=np.int64)) == 0
    assert out.min() == out.max() == -1
    # no group: the sums are empty
    assert call(g=0, lo=np.array([0], dtype=np.int64), ao=np.array([0], dtype=np.int64)) == 0 and out[0, 0].tolist() == [0, 0, 0, 0]
    assert call() == 0 and np.array_equal(out, keep)


def test_list_overflow_is_refused_by_track(ctx):
    """a sum that could leave 64 bits is refused, never computed: by the track's own size for any list, and by the number of
    segments times it for lists that are not normalized"""
    L = _lib.lib()
    big = overflow_track()[0]
    small = [([(10, 20)], [Q_MAX]), ([(5, 25)], [-Q_MAX])]                    # the same values over short pieces
    normalized = [[[(0, 100)], [(0, 100)]]]
    assert device_words(ctx, normalized, [small, small]).tolist() == [[[2, 30, 2, -10 * Q_MAX]] * 2]
    with pytest.raises(ValueError, match="signal track 1:.*2\\^63") as e:
        device_words(ctx, normalized, [small, big])
    assert "signal track 0" not in str(e.value)
    # one of the two groups alone stays below 2^63: a normalized list is taken, and the sum is exact
    half = [big[0], ([], [])]
    assert device_words(ctx, normalized, [half]).tolist() == [[[2, 100, 1, 100 * Q_MAX]]]
    assert device_words(ctx, [[[(0, 2 ** 31)], []]], [half])[0, 0].tolist() == [1, 2 ** 31, 1, Q_MAX * 2 ** 31]
    # ... a list that is not normalized could count its bases twice: three overlapping segments x M pass 2^63
    overlapping = [[[(0, 100), (50, 150), (60, 70)], []]]
    with pytest.raises(ValueError, match="signal track 0:.*not normalized.*2\\^63"):
        device_words(ctx, overlapping, [half])
    assert device_words(ctx, overlapping, [small])[0, 0].tolist() == M.pair_words(overlapping[0], small)
    out = np.full((1, 1, 4), -1, dtype=np.int64)
    a, a_off = csr(normalized)
    pc, v, p_off = track_csr([big])
    assert L.gat_list_signal(ctx._h, _lib._p(a), _lib._p(a_off), 1, _lib._p(pc), _lib._p(v), _lib._p(p_off), 1, 2, _lib._p(out)) == ERR_ARG
    assert out.min() == out.max() == -1


# ---- 2. gat_sample_signal -----------------------------------------------------------------------------------------------------------
SEED, SAMPLES = 77, 12
UNSORTED = ("segments-units", "segments-genome")               # SamplerSegments without isochore keys


def tracks_for(flat, seed=5):
    """three small tracks over the contigs of a problem: a few pieces, a dozen, and one of up to 70 that is empty on the last
    contig; values in [-5, 5]"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = []
    for k in (3, 12, 70):
        per = []
        for c in range(len(ext)):
            pieces, values = M.random_pieces(r, k, max(50, int(ext[c])), max_len=9)
            keep = [i for i, (a, b) in enumerate(pieces) if b < 2 ** 32]
            per.append(([pieces[i] for i in keep], [values[i] for i in keep]))
        tracks.append(per)
    tracks[2][len(ext) - 1] = ([], [])
    return tracks


@pytest.fixture(scope="module")
def six(ctx):
    """per problem of CC.SIX: the flat problem, its tracks, Problem.sample of (SEED, 0, SAMPLES) -- drawn once"""
    cache = {}

    def get(name):
        if name not in cache:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            try:
                seg, off = P.sample(SEED, 0, SAMPLES)
            finally:
                P.close()
            cache[name] = (flat, tracks_for(flat), seg, off)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(CC.SIX))
def test_six_samplers(ctx, six, name):
    flat, tracks, seg, off = six(name)
    pieces, vals, piece_off = track_csr(tracks)
    P = _lib.Problem(ctx, flat)
    try:
        normalized = all(M.is_normalized(seg[off[l]:off[l + 1]]) for l in range(len(off) - 1))
        assert normalized == (name not in UNSORTED)
        want = M.from_sample(seg, off, P.n_contigs, tracks)
        got = P.sample_signal(SEED, 0, SAMPLES, pieces, vals, piece_off, 3)
        assert got.dtype == np.int64 and got.shape == (SAMPLES, 3, 4)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
        assert got[:, :, 0].min() > 0 and got[:, :, 1].sum() > 0 and (got[:, :, 0] == got[:, :1, 0]).all()
        # split invariance: [0, 12) is [0, 5) followed by [5, 12)
        a = P.sample_signal(SEED, 0, 5, pieces, vals, piece_off, 3)
        b = P.sample_signal(SEED, 5, SAMPLES, pieces, vals, piece_off, 3)
        assert np.array_equal(np.concatenate([a, b]), got)
    finally:
        P.close()


def test_many_batches(ctx, monkeypatch):
    """a scratch budget of a few samples: the range goes through in several batches, the words are those of one"""
    flat = CC.genome_problem(CC.ANNOTATOR, True)
    tracks = tracks_for(flat)
    pieces, vals, piece_off = track_csr(tracks)
    P = _lib.Problem(ctx, flat)
    try:
        whole = P.sample_signal(8, 0, 24, pieces, vals, piece_off, 3)
        assert P.last_stats["n_batches"] == 1
        seg, off = P.sample(8, 0, 24)
        assert np.array_equal(whole, M.from_sample(seg, off, P.n_contigs, tracks))
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, flat)
    try:
        cut = P.sample_signal(8, 0, 24, pieces, vals, piece_off, 3)
        assert P.last_stats["n_batches"] > 3, P.last_stats["n_batches"]
        assert np.array_equal(cut, whole)
    finally:
        P.close()


def test_sample_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    flat = CC.unit_problem("annotator")
    tracks = tracks_for(flat)
    pieces, vals, piece_off = track_csr(tracks)
    P = _lib.Problem(ctx, flat)
    try:
        C_ = P.n_contigs
        out = np.full((2, 3, 4), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, a=pieces, v=vals, ao=piece_off, t=3, o=out):
            return L.gat_sample_signal(c, prob, 5, begin, end, p(a), p(v), p(ao), t, p(o), None)

        assert call() == 0 and out[:, :, :3].min() >= 0
        keep = out.copy()
        out[:] = -1
        down = piece_off.copy()
        down[1] = down[2] + 1
        low = vals.copy()
        low[len(low) // 2] = INT32_MIN
        for bad in (dict(c=None), dict(prob=None), dict(ao=None), dict(o=None), dict(a=None), dict(v=None), dict(begin=3, end=2), dict(t=-1),
                    dict(ao=down), dict(v=low)):
            assert call(**bad) == ERR_ARG, bad
            assert out.min() == out.max() == -1, bad
        assert b"INT32_MIN" in L.gat_last_error(ctx._h)
        # an unnormalized track is named: track 1, the problem's contig 2
        bad_pieces = pieces.copy()
        at = int(piece_off[1 * C_ + 2])
        assert piece_off[1 * C_ + 2 + 1] - at >= 2
        bad_pieces["start"][at + 1] = bad_pieces["end"][at] - 1
        assert call(a=bad_pieces) == ERR_ARG and b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h)
        # the overflow bound, by track: track 1 of 2 is the one whose sum over the contigs passes 2^63
        assert C_ >= 2
        big = [overflow_track()[0] + [([], [])] * (C_ - 2)]
        bp, bv, bo = track_csr([tracks[0]] + big)
        out2 = np.full((2, 2, 4), -1, dtype=np.int64)
        assert call(a=bp, v=bv, ao=bo, t=2, o=out2) == ERR_ARG and out2.min() == out2.max() == -1
        assert b"signal track 1:" in L.gat_last_error(ctx._h) and b"2^63" in L.gat_last_error(ctx._h)
        bv[np.abs(bv.astype(np.int64)) == Q_MAX] = 7                                  # (the same long pieces with small values are taken)
        assert call(a=bp, v=bv, ao=bo, t=2, o=out2) == 0 and np.array_equal(out2[:, 0], keep[:, 0])
        assert out.min() == out.max() == -1
        assert call(begin=4, end=4) == 0 and call(t=0, ao=np.array([0], dtype=np.int64)) == 0      # an empty range, no track: nothing written
        assert out.min() == out.max() == -1
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], 5, 0, 2, dev)
            assert call() == ERR_ARG and b"in flight" in L.gat_last_error(ctx._h)
            P.wait()
        finally:
            ctx.free(dev)
        assert out.min() == out.max() == -1
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()


def test_unsorted_sampled_lists_take_the_other_bound(ctx):
    """SamplerSegments without isochore keys: the lists are not normalized, a base may count once per segment -- a track that a
    problem with normalized lists takes is refused there, by what the slab holds; the same piece with a small value is taken"""
    heavy = lambda C_: [[([(0, 2 ** 31)], [Q_MAX])] + [([], [])] * (C_ - 1)]          # noqa: E731  (M = 2^62 - 2^31)
    for sampler, refused in ((CC.SEGMENTS, True), (CC.ANNOTATOR, False)):
        P = _lib.Problem(ctx, CC.genome_problem(sampler, False))
        try:
            C_ = P.n_contigs
            pieces, vals, off = track_csr(heavy(C_))
            seg, soff = P.sample(SEED, 0, 4)
            if refused:
                with pytest.raises(ValueError, match="signal track 0:.*not normalized.*2\\^63"):
                    P.sample_signal(SEED, 0, 4, pieces, vals, off, 1)
                vals[:] = 3
            got = P.sample_signal(SEED, 0, 4, pieces, vals, off, 1)
            want = M.from_sample(seg, soff, C_, [[(g[0], vals[:len(g[0])].tolist()) for g in heavy(C_)[0]]])
            assert np.array_equal(got, want) and np.array_equal(got[:, 0, 3], int(vals[0]) * got[:, 0, 1]) and got[:, 0, 1].sum() > 0
        finally:
            P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        pieces, vals, off = track_csr([[([(1, 2)], [4]) for _ in range(P.n_contigs)]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_signal(1, 0, 1, pieces, vals, off, 1)
        assert P.last_stats["n_unconverged"] == 1
    finally:
        P.close()


# ---- 3. the script ------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES, CLI_SCALE = 11, 50, 1000


def write_bedgraphs(tmp_path):
    """two signal files over the contigs of tests/golden/cli: pieces of a few hundred bases with gaps, values of three decimals,
    negative ones among them; one gzipped, one with header lines"""
    import gzip
    r = random.Random(9)
    paths = []
    for name, lo, hi, opener in (("cons.bedGraph", 0.0, 1.0, open), ("delta.bg.gz", -2.0, 2.0, gzip.open)):
        path = str(tmp_path / name)
        with opener(path, "wt") as f:
            f.write("track type=bedGraph name=%s\n# made by the test\n" % name)
            for contig in ("chrD", "chrA", "chrB", "chrC", "chrUn"):
                pos = r.randint(0, 500)
                while pos < 400000:
                    ln = r.randint(50, 900)
                    f.write("%s\t%d\t%d\t%.3f\n" % (contig, pos, pos + ln, r.uniform(lo, hi)))
                    pos += ln + r.choice([0, 0, r.randint(1, 2000)])
        paths.append(path)
    return paths


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed")],
                                   ["--with-segment-tracks", "--counter=signal-mean", "--counter=signal-hit"],
                                   ["--sampler=circular", "--counter=signal-mean", "--counter=signal-hit"]],
                         ids=["isochores", "tracks-two-counters", "circular-two-counters"])
def test_script(ctx, tmp_path, extra):
    """the printed tables are the ones built here: Problem.sample of the same inputs and seeds, the model, engine.AnnotatorResult,
    IO.outputResults"""
    import optparse
    from gat_amd import engine, problem, signals
    from gat_amd import io as IO
    from test_signal_host import script
    mod = script()
    pattern = str(tmp_path / "got.%s.tsv")
    files = write_bedgraphs(tmp_path)
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--workspace=%s" % os.path.join(CLI, "workspace.bed")] + \
           ["--signal=%s" % f for f in files] + \
           ["--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED, "--verbose=0", "--output-tables-pattern=%s" % pattern] + extra
    assert mod.main(["gat-signal.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    # the model: the same inputs, the lists of the same seeds
    opts, _ = mod.buildParser().parse_args(argv)
    counters = opts.counters or ["signal-mean"]
    assert opts.pseudo_count == 0
    segments, workspace = signals.build_inputs(opts)
    sig = signals.read_tracks(files, CLI_SCALE)
    names = [t.name for t in sig]
    assert names == ["cons", "delta"] and len(segments.tracks) == (2 if "--with-segment-tracks" in extra else 1)
    results = {c: [] for c in counters}
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, _ = signals.flatten(segments[track], workspace, signals.make_sampler(opts))
        contigs = list(flat["contig_names"])
        assert ("--isochores" in extra[0]) == bool(flat["merge_contigs"]) and "chrUn" not in contigs
        csegs = problem.from_isochores(sa)
        tracks = [[(t.pieces[c][0], t.pieces[c][1].tolist()) if c in t.pieces else ([], []) for c in contigs] for t in sig]
        observed_lists = [[csegs.get(c, []) for c in contigs]]
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        obs = M.all_words(observed_lists, tracks)[0]
        null = M.from_sample(seg, off, len(contigs), tracks)
        for c in counters:
            value = (lambda w: float(w[2])) if c == "signal-hit" else (lambda w: w[3] / w[1] / CLI_SCALE if w[1] else 0.0)
            for t, a in enumerate(names):
                results[c].append(engine.AnnotatorResult(track, a, c, value(obs[t].tolist()), [value(w) for w in null[:, t].tolist()],
                                                         pseudo_count=0.0))
    want = {}
    if len(counters) == 1:
        sink = io.StringIO()
        IO.outputResults(results[counters[0]], optparse.Values(dict(vars(opts), stdout=sink)), engine.AnnotatorResult.headers,
                         format_observed="%6.4f")
        want[str(tmp_path / "got.tsv")] = sink.getvalue()
    else:
        wpattern = str(tmp_path / "want.%s.tsv")
        IO.outputResults([r for c in counters for r in results[c]], optparse.Values(dict(vars(opts), output_tables_pattern=wpattern)),
                         engine.AnnotatorResult.headers, format_observed="%6.4f")
        for c in counters:
            want[pattern % c] = open(wpattern % c).read()
    for path, text in want.items():
        got = "".join(l for l in open(path) if not l.startswith("#"))
        assert got == text, path
        rows = [l.split("\t") for l in text.splitlines()[1:]]
        assert len(rows) == len(names) * len(segments.tracks) and all(len(r) == 11 for r in rows)
        assert any(float(r[3]) != 0 for r in rows)              # (an expected value: the null is not empty)
