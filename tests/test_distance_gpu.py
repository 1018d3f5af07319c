"""GPU: k_distance.  gat_list_distances against the model (tests/distance_model.py) on the hand cases and on lists around the
lane-stride and staging edges, gat_sample_distances against the model applied to Problem.sample of the SAME problem, seed and
sample range, and scripts/gat-distance.py against the table built here from Problem.sample, the model and
engine.AnnotatorResult.  Every comparison is exact: integers, or the text of a table."""
import io
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import distance_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
DIRECTIONS = (M.SEGMENT_TO_ANNOTATION, M.ANNOTATION_TO_SEGMENT)
BOUNDS = (0, 1, 2 ** 32)
LDS = ("default", "8")                  # GAT_DISTANCE_LDS_PIECES: lists of 9 intervals and more end in global memory at 8


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(params=LDS)
def lds(request, ctx, monkeypatch):
    if request.param != "default":
        monkeypatch.setitem(ctx.options, "GAT_DISTANCE_LDS_PIECES", request.param)
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


def device_words(ctx, lists, tracks, direction, max_distance):
    """lists[l][g] and tracks[t][g] -> int64 [n_lists, n_tracks, 4] from gat_list_distances"""
    n_groups = len(lists[0]) if lists else len(tracks[0])
    a, a_off = csr(lists)
    b, b_off = csr(tracks)
    return _lib.list_distances(ctx, a, a_off, len(lists), b, b_off, len(tracks), n_groups, direction, max_distance)


def check(ctx, searched, queries, direction, max_distance, what=""):
    """searched[i][g]: normalized lists, queries[k][g]: any lists.  Direction 0: the queries are the segment lists and the
    searched lists the tracks; direction 1 the other way round.  Returns the words as [query][searched][4]."""
    lists, tracks = (queries, searched) if direction == M.SEGMENT_TO_ANNOTATION else (searched, queries)
    got = device_words(ctx, lists, tracks, direction, max_distance)
    want = M.all_words(lists, tracks, direction, max_distance)
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, direction, max_distance, bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    return got if direction == M.SEGMENT_TO_ANNOTATION else got.transpose(1, 0, 2)


# ---- 1. gat_list_distances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_hand_cases(ctx, lds, direction):
    """every hand case's queries against every hand case's T (most of them not made for each other), one group, at the three
    bounds; the pairs that were made for each other give the distances written beside them"""
    cases = M.HAND + [M.EMPTY_T]
    searched = [[t] for _, _, t, _ in cases]
    queries = [[q] for _, q, _, _ in cases]
    for bound in BOUNDS + (40,):
        got = check(ctx, searched, queries, direction, bound, "hand")
        for i, (name, _, _, want) in enumerate(M.HAND):
            assert got[i, i].tolist() == [len(want), sum(want), sum(1 for d in want if d <= bound), 0], (name, bound)
        assert got[len(M.HAND), len(M.HAND)].tolist() == M.EMPTY_T[3]
    assert got[:, :, 1].max() > 2 ** 32 and got[:, :, 3].sum() > 0             # (a sum beyond 32 bits; queries without a neighbour)


T_SIZES = (0, 1, 2, 8, 9, 63, 64, 65, 129)
Q_SIZES = (0, 1, 63, 64, 65, 129)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_list_sizes(ctx, lds, direction):
    """searched lists around the staging limit and its blocks (8, 9, 64, 65 at a limit of 8), query lists around one and two
    rounds of 64 lanes: every pair, in one launch"""
    r = random.Random(7)
    searched = [[M.random_normalized(r, k, 3000)] for k in T_SIZES]
    assert [len(s[0]) for s in searched] == list(T_SIZES)
    top = max(s[0][-1][1] for s in searched if s[0])
    queries = [[M.random_queries(r, n, top + 200)] for n in Q_SIZES]
    for k in (1, 3):                                            # every interval itself, its left and its right neighbour base
        t = searched[T_SIZES.index(65)][0]
        queries.append([[(a, b) for a, b in t] + [(a - k, a) for a, _ in t if a >= k] + [(b, b + k) for _, b in t]])
    got = check(ctx, searched, queries, direction, 25, "sizes")
    assert got[:, 1:, 0].sum() > 0 and got[:, 0, 3].sum() > 0 and (got[:, :, 2] < got[:, :, 0]).any()


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("n_tracks", [1, 2, 5])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_tracks_and_groups(ctx, lds, direction, n_tracks, n_groups):
    """the sums over the groups: seven segment lists, 1 / 2 / 5 tracks, 1 / 3 groups; with three groups one track is empty
    on one group and one list on another"""
    r = random.Random(100 * n_tracks + n_groups)
    normalized = lambda: [M.random_normalized(r, r.choice([1, 3, 20, 70]), 2000) for _ in range(n_groups)]      # noqa: E731
    anyhow = lambda: [M.random_queries(r, r.choice([1, 5, 70]), 2500) for _ in range(n_groups)]                  # noqa: E731
    lists = [normalized() if direction == M.ANNOTATION_TO_SEGMENT else anyhow() for _ in range(7)]
    tracks = [anyhow() if direction == M.ANNOTATION_TO_SEGMENT else normalized() for _ in range(n_tracks)]
    if n_groups > 1:
        tracks[n_tracks - 1][n_groups - 1] = []
        lists[2][0] = []
    searched, queries = (tracks, lists) if direction == M.SEGMENT_TO_ANNOTATION else (lists, tracks)
    got = check(ctx, searched, queries, direction, 30, "groups")
    assert got[:, :, 0].sum() > 0 and (n_groups == 1 or got[:, :, 3].sum() > 0)


def test_staging_limit_changes_no_result(ctx, monkeypatch):
    r = random.Random(3)
    searched = [[M.random_normalized(r, k, 20000)] for k in (1, 64, 65, 200, 1000)]
    queries = [[M.random_queries(r, 150, 22000)] for _ in range(5)]
    want = check(ctx, searched, queries, 0, 100)
    for limit in ("1", "7", "200", "2048", "100000000"):
        monkeypatch.setitem(ctx.options, "GAT_DISTANCE_LDS_PIECES", limit)
        assert np.array_equal(check(ctx, searched, queries, 0, 100), want), limit
        assert np.array_equal(check(ctx, searched, searched, 1, 100), check(ctx, searched, searched, 0, 100)), limit


def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, annos = seg_array([(1, 5), (30, 40)]), seg_array([(0, 4), (4, 8), (20, 22)])
    off, aoff = np.array([0, 2], dtype=np.int64), np.array([0, 3], dtype=np.int64)
    out = np.full((1, 1, 4), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, a=annos, ao=aoff, t=1, g=1, d=0, m=10, o=out):
        return L.gat_list_distances(c, p(lists), p(lo), n, p(a), p(ao), t, g, d, m, p(o))

    assert call() == 0 and out[0, 0].tolist() == M.words([(1, 5), (30, 40)], [(0, 4), (4, 8), (20, 22)], 10) == [2, 9, 2, 0]
    assert call(d=1) == 0 and out[0, 0].tolist() == M.words([(0, 4), (4, 8), (20, 22)], [(1, 5), (30, 40)], 10) == [3, 9, 3, 0]
    down = np.array([2, 0], dtype=np.int64)
    for bad in (dict(c=None), dict(lo=None), dict(ao=None), dict(o=None), dict(lists=None), dict(a=None), dict(n=-1), dict(t=-1),
                dict(g=-1), dict(lo=down), dict(ao=np.array([3, 0], dtype=np.int64)), dict(d=2), dict(d=-1), dict(m=-1), dict(m=2 ** 32 + 1)):
        assert call(**bad) == -6, bad
    # the searched side must be normalized: the tracks in direction 0, the segment lists in direction 1 -- and only that side
    for bad in (seg_array([(0, 4), (3, 8), (20, 22)]), seg_array([(4, 8), (0, 4), (20, 22)]), seg_array([(0, 4), (6, 6), (20, 22)])):
        assert call(a=bad) == -6 and b"annotation track 0, group 0 is not normalized" in L.gat_last_error(ctx._h)
        assert call(lists=bad, lo=aoff, d=1) == -6 and b"segment list 0, group 0 is not normalized" in L.gat_last_error(ctx._h)
        assert call(a=bad, d=1) == 0 and call(lists=bad, lo=aoff) == 0
    # ... and the message names the track and the group: track 1 of 2, group 2 of 3
    a6, o6 = csr([[[(0, 4)], [], [(5, 6)]], [[(1, 2)], [(3, 4)], [(9, 12), (11, 13)]]])
    l3, lo3 = csr([[[(0, 4)], [(2, 3)], []]])
    out2 = np.full((1, 2, 4), -1, dtype=np.int64)
    assert call(lists=l3, lo=lo3, a=a6, ao=o6, t=2, g=3, o=out2) == -6
    assert b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h)
    assert out2.min() == -1
    # nothing to compare: nothing written
    keep = out.copy()
    assert call(n=0, lo=np.array([0], dtype=np.int64)) == 0 and call(t=0, ao=np.array([0], dtype=np.int64)) == 0
    assert np.array_equal(out, keep)
    # no group: the sums are empty
    assert call(g=0, lo=np.array([0], dtype=np.int64), ao=np.array([0], dtype=np.int64)) == 0 and out[0, 0].tolist() == [0, 0, 0, 0]


# ---- 2. gat_sample_distances --------------------------------------------------------------------------------------------------------
SEED, SAMPLES, BOUND = 77, 12, 50
UNSORTED = ("segments-units", "segments-genome")               # SamplerSegments without isochore keys


def tracks_for(flat, seed=5):
    """three small tracks over the contigs of a problem: a few intervals, a dozen, and one of up to 70 that is empty on the
    last contig"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = []
    for k in (3, 12, 70):
        per = []
        for c in range(len(ext)):
            t = M.random_normalized(r, k, max(50, int(ext[c])), max_len=9)
            per.append([(a, b) for a, b in t if b < 2 ** 32])
        tracks.append(per)
    tracks[2][len(ext) - 1] = []
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


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("name", sorted(CC.SIX))
def test_six_samplers(ctx, six, name, direction):
    flat, tracks, seg, off = six(name)
    annos, anno_off = csr(tracks)
    P = _lib.Problem(ctx, flat)
    try:
        C_ = P.n_contigs
        if direction == M.ANNOTATION_TO_SEGMENT and name in UNSORTED:
            with pytest.raises(ValueError, match="not normalized"):
                P.sample_distances(SEED, 0, SAMPLES, annos, anno_off, 3, direction, BOUND)
            return
        if direction == M.ANNOTATION_TO_SEGMENT:
            assert all(M.is_normalized(seg[off[l]:off[l + 1]]) for l in range(len(off) - 1))
        want = M.from_sample(seg, off, C_, tracks, direction, BOUND)
        got = P.sample_distances(SEED, 0, SAMPLES, annos, anno_off, 3, direction, BOUND)
        assert got.dtype == np.int64 and got.shape == (SAMPLES, 3, 4)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
        assert got[:, :, 0].sum() > 0 and got[:, :, 1].sum() > 0
        assert direction == M.ANNOTATION_TO_SEGMENT or got[:, 2, 3].sum() > 0     # (the track that is empty on the last contig)
        # split invariance: [0, 12) is [0, 5) followed by [5, 12)
        a = P.sample_distances(SEED, 0, 5, annos, anno_off, 3, direction, BOUND)
        b = P.sample_distances(SEED, 5, SAMPLES, annos, anno_off, 3, direction, BOUND)
        assert np.array_equal(np.concatenate([a, b]), got)
    finally:
        P.close()


def test_unsorted_lists_are_what_the_problems_say(six):
    """the lists direction 1 refuses are not normalized indeed, and direction 0 has counted queries that overlap each other"""
    for name in UNSORTED:
        _, _, seg, off = six(name)
        assert not all(M.is_normalized(seg[off[l]:off[l + 1]]) for l in range(len(off) - 1)), name


def test_many_batches(ctx, monkeypatch):
    """a scratch budget of a few samples: the range goes through in several batches, the words are those of one"""
    flat = CC.genome_problem(CC.ANNOTATOR, True)
    tracks = tracks_for(flat)
    annos, anno_off = csr(tracks)
    whole = {}
    P = _lib.Problem(ctx, flat)
    try:
        for d in DIRECTIONS:
            whole[d] = P.sample_distances(8, 0, 24, annos, anno_off, 3, d, BOUND)
            assert P.last_stats["n_batches"] == 1
        seg, off = P.sample(8, 0, 24)
        for d in DIRECTIONS:
            assert np.array_equal(whole[d], M.from_sample(seg, off, P.n_contigs, tracks, d, BOUND))
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, flat)
    try:
        for d in DIRECTIONS:
            cut = P.sample_distances(8, 0, 24, annos, anno_off, 3, d, BOUND)
            assert P.last_stats["n_batches"] > 3, P.last_stats["n_batches"]
            assert np.array_equal(cut, whole[d])
    finally:
        P.close()


def test_sample_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    flat = CC.unit_problem("annotator")
    tracks = tracks_for(flat)
    annos, anno_off = csr(tracks)
    P = _lib.Problem(ctx, flat)
    try:
        C_ = P.n_contigs
        out = np.full((2, 3, 4), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, a=annos, ao=anno_off, t=3, d=0, m=BOUND, o=out):
            return L.gat_sample_distances(c, prob, 5, begin, end, p(a), p(ao), t, d, m, p(o), None)

        assert call() == 0 and out.min() >= 0
        keep = out.copy()
        down = anno_off.copy()
        down[1] = down[2] + 1
        for bad in (dict(c=None), dict(prob=None), dict(ao=None), dict(o=None), dict(a=None), dict(begin=3, end=2), dict(t=-1), dict(ao=down),
                    dict(d=2), dict(m=-1), dict(m=2 ** 32 + 1)):
            assert call(**bad) == -6, bad
        # an unnormalized track is named: track 1, the problem's contig 2
        bad_annos = annos.copy()
        at = int(anno_off[1 * C_ + 2])
        assert anno_off[1 * C_ + 2 + 1] - at >= 2
        bad_annos["start"][at + 1] = bad_annos["end"][at] - 1
        assert call(a=bad_annos) == -6 and b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h)
        assert call(a=bad_annos, d=1) == 0                       # (the queries of direction 1 may be any list)
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == -1          # an empty range writes nothing
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], 5, 0, 2, dev)
            assert call() == -6 and b"in flight" in L.gat_last_error(ctx._h)
            P.wait()
        finally:
            ctx.free(dev)
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()
    # the sampler whose lists direction 1 cannot search
    P = _lib.Problem(ctx, CC.genome_problem(CC.SEGMENTS, False))
    try:
        t2 = tracks_for(CC.genome_problem(CC.SEGMENTS, False))
        a2, o2 = csr(t2)
        out = np.full((2, 3, 4), -1, dtype=np.int64)
        assert L.gat_sample_distances(ctx._h, P._h, 5, 0, 2, p(a2), p(o2), 3, 1, BOUND, p(out), None) == -6
        assert b"not normalized" in L.gat_last_error(ctx._h) and out.min() == out.max() == -1
        assert L.gat_sample_distances(ctx._h, P._h, 5, 0, 2, p(a2), p(o2), 3, 0, BOUND, p(out), None) == 0 and out.min() >= 0
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        annos, anno_off = csr([[[(1, 2)] for _ in range(P.n_contigs)]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_distances(1, 0, 1, annos, anno_off, 1, 0, BOUND)
        assert P.last_stats["n_unconverged"] == 1
    finally:
        P.close()


# ---- 3. the script ------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES, CLI_BOUND = 11, 50, 300
ALL_COUNTERS = ["--counter=segment-distance", "--counter=segment-nearby", "--counter=annotation-distance", "--counter=annotation-nearby"]


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed")], ["--with-segment-tracks"] + ALL_COUNTERS,
                                   ["--sampler=circular"] + ALL_COUNTERS],
                         ids=["isochores", "tracks-four-counters", "circular-four-counters"])
def test_script(ctx, tmp_path, extra):
    """the printed tables are the ones built here: Problem.sample of the same inputs and seeds, the model, engine.AnnotatorResult,
    IO.outputResults"""
    import optparse
    from gat_amd import distance, engine, problem
    from gat_amd import io as IO
    from test_distance_host import script
    mod = script()
    pattern = str(tmp_path / "got.%s.tsv")
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--max-distance=%d" % CLI_BOUND, "--verbose=0", "--output-tables-pattern=%s" % pattern] + extra
    assert mod.main(["gat-distance.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    # the model: the same inputs, the lists of the same seeds
    opts, _ = mod.buildParser().parse_args(argv)
    counters = opts.counters or ["segment-distance"]
    segments, annotations, workspace = distance.build_inputs(opts)
    names = list(annotations.tracks)
    assert len(names) >= 2
    results = {c: [] for c in counters}
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, _ = distance.flatten(segments[track], workspace, distance.make_sampler(opts))
        contigs = list(flat["contig_names"])
        assert ("--isochores" in extra[0]) == bool(flat["merge_contigs"])
        csegs = problem.from_isochores(sa)
        tracks = []
        for t in names:
            per = problem.from_isochores(annotations[t].asArrays())
            tracks.append([per[c] if c in per else [] for c in contigs])
        observed_lists = [[csegs.get(c, []) for c in contigs]]
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        for c in counters:
            d, what = distance.COUNTERS[c]
            obs = M.all_words(observed_lists, tracks, d, CLI_BOUND)[0]
            null = M.from_sample(seg, off, len(contigs), tracks, d, CLI_BOUND)
            for t, a in enumerate(names):
                value = (lambda w: float(w[2]) if what == "near" else (w[1] / w[0] if w[0] else 0.0))
                results[c].append(engine.AnnotatorResult(track, a, c, value(obs[t].tolist()), [value(w) for w in null[:, t].tolist()]))
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
        assert any(float(r[3]) > 0 for r in rows)               # (an expected value: the null is not empty)
