"""GPU: k_pairs.  gat_list_pair_hits against the model (tests/pairs_model.py) on hand-made geometry at every tile shape and three
staging limits, gat_sample_pair_enrichment against the model applied to Problem.sample of the SAME problem, seed and sample
range, its diagonal against the count stage's segment-overlap, and scripts/gat-pairs.py against the table built here from
Problem.sample and the model.  Every comparison is exact: integers, or the text of a table."""
import io
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import pairs_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
TRACKS = (1, 2, 63, 64, 65, 130)        # one tile; a partial one; a full one; diagonal + off-diagonal; a partial off-diagonal
PIECES = ("default", "4", "0")          # GAT_PAIRS_LDS_PIECES: a track of 5 intervals and more ends in global memory at 4; 0: all of it
RUNS = ("default", "1", "5")            # GAT_PAIRS_SAMPLES_PER_BLOCK
TOP = 2 ** 32 - 1
WORDS = 5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_options(ctx, monkeypatch, **options):
    for key, value in options.items():
        if value != "default":
            monkeypatch.setitem(ctx.options, key, value)
        else:
            monkeypatch.delitem(ctx.options, key, raising=False)


def pair_of(i, j, T):
    return i * T - i * (i - 1) // 2 + (j - i)


# ---- 1. gat_list_pair_hits ------------------------------------------------------------------------------------------------------------
def mixed_geometry():
    """130 tracks and 6 lists over 3 groups; group 1 holds no interval of any track"""
    r = random.Random(41)
    tracks = [
        [[(10, 20), (20, 30), (50, 60)], [], [(TOP - 1, TOP)]],                                  # adjacent intervals; the last base there is
        [[], [], []],                                                                            # an empty track
        [[(7 * i, 7 * i + 3) for i in range(40)], [], [(0, 50)]],                                # longer than a staging limit of 4
    ]
    for t in range(3, 130):
        tracks.append([M.random_normalized(r, r.choice([1, 3, 9, 20]), 300, 20), [], M.random_normalized(r, r.choice([0, 2]), 300, 40)])
    unsorted = [(s, s + r.choice([1, 2, 9, 60])) for s in (r.randrange(0, 320) for _ in range(64))]
    more = [(s, s + r.choice([1, 3, 30])) for s in (r.randrange(0, 320) for _ in range(39))]
    lists = [
        # bookended on either side of an interval (no hit) next to one shared base (a hit); a segment over several intervals
        [[(0, 10), (0, 11), (30, 50), (29, 30), (60, 61), (59, 60), (5, 100)], [(3, 9)], [(TOP - 2, TOP - 1), (TOP - 1, TOP), (0, TOP)]],
        [[], [], []],                                                                            # an empty list
        [[(15, 16)], [], []],                                                                    # one segment
        [unsorted, [], []],                                                                      # 64, unsorted and overlapping
        [more + [(18, 12), (15, 15)], [(0, 400)], [(s, s + 25) for s in range(0, 299, 13)]],    # 65; a reversed and an empty segment
        [[(0, 400), (1000, 1001)], [], [(0, TOP)]],                                              # over every interval; beyond all
    ]
    return tracks, lists


def dense_geometry():
    """130 tracks that all hold an interval below 400 in group 0: a segment hits all of them, one hits none, and short segments
    hit a few neighbours each"""
    tracks = [[[(3 * t + 1, 3 * t + 3), (500 + 5 * t, 502 + 5 * t)], [(t, t + 1)] if t % 2 else []] for t in range(130)]
    lists = [
        [[(0, 400), (450, 460)], []],
        [[(3 * t + 2, 3 * t + 8) for t in range(0, 130, 3)] + [(0, 400)], [(60, 70), (0, 130)]],
        [[(400, 2000)], [(129, 130)]],
    ]
    return tracks, lists


GEOMETRIES = {"mixed": mixed_geometry, "dense": dense_geometry}


@pytest.fixture(scope="module")
def geometry():
    """per geometry: tracks, lists and the model's counts for every T of TRACKS, computed once"""
    out = {}
    for name, make in GEOMETRIES.items():
        tracks, lists = make()
        out[name] = dict(tracks=tracks, lists=lists, want={T: M.all_counts(lists, tracks[:T]) for T in TRACKS})
    return out


def test_hand_geometry_is_what_it_says(geometry):
    g = geometry["mixed"]
    tracks, lists = g["tracks"], g["lists"]
    assert all(M.is_normalized(a) for t in tracks for a in t) and all(len(t[1]) == 0 for t in tracks) and not any(tracks[1])
    assert [sum(len(x) for x in l) for l in lists] == [11, 0, 1, 64, 65, 3]
    assert not M.is_normalized(lists[3][0])
    assert max(e for l in lists for x in l for _, e in x) == TOP and len(tracks[2][0]) == 40
    w = g["want"][130]
    k = lambda i, j: pair_of(i, j, 130)                                                      # noqa: E731
    # list 0 against track 0: (0, 11), (29, 30), (59, 60), (5, 100) in group 0; (TOP - 1, TOP) and (0, TOP) in group 2
    assert w[0, k(0, 0)] == 6 and w[1].sum() == 0 and w[:, k(1, 1)].sum() == 0
    assert M.hits(lists[0][0], tracks[0][0]).tolist() == [False, True, False, True, False, True, True]
    d = geometry["dense"]
    assert M.hit_matrix(d["lists"][0], d["tracks"]).sum(axis=1).tolist() == [130, 0]


@pytest.mark.parametrize("T", TRACKS)
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_list_pair_hits(ctx, monkeypatch, geometry, name, T):
    """the model's counts, whatever the staging limit and the run"""
    g = geometry[name]
    tracks, lists, want = g["tracks"][:T], g["lists"], g["want"][T]
    G = len(lists[0])
    assert G <= 3 and all(len(l) == G and sum(len(x) for x in l) <= 200 for l in lists)
    # the premises: something is counted; with more than one block, in an off-diagonal tile; in a partial tile where there is one;
    # and some pair is hit together less often than either of its tracks
    assert want.sum() > 0
    c = want.sum(axis=0)
    if T > 64:
        assert any(c[pair_of(i, j, T)] > 0 for i in range(64) for j in range(64, T))
    if T % 64:
        assert any(c[pair_of(i, j, T)] > 0 for j in range(T - T % 64, T) for i in range(j + 1))
    if T > 2:
        assert any(0 < l[pair_of(i, j, T)] < min(l[pair_of(i, i, T)], l[pair_of(j, j, T)]) for l in want for i in range(T) for j in range(i + 1, T))
    a, a_off = M.csr(lists)
    b, b_off = M.csr(tracks)
    for pieces in PIECES:
        for run in ("default", "1"):
            set_options(ctx, monkeypatch, GAT_PAIRS_LDS_PIECES=pieces, GAT_PAIRS_SAMPLES_PER_BLOCK=run)
            got = ctx.list_pair_hits(a, a_off, len(lists), b, b_off, T, G)
            assert got.dtype == np.int64 and got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (name, T, pieces, run, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, annos = _lib_seg([(1, 5), (30, 40), (8, 9)]), _lib_seg([(0, 4), (4, 8), (20, 32)])
    off, aoff = np.array([0, 3], dtype=np.int64), np.array([0, 3], dtype=np.int64)
    out = np.full((1, 1), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, a=annos, ao=aoff, t=1, g=1, o=out):
        return L.gat_list_pair_hits(c, p(lists), p(lo), n, p(a), p(ao), t, g, p(o))

    assert call() == 0 and out.tolist() == [[2]]
    keep = out.copy()
    for bad in (dict(c=None), dict(lo=None), dict(ao=None), dict(o=None), dict(lists=None), dict(a=None), dict(n=-1), dict(t=-1), dict(g=-1),
                dict(lo=np.array([2, 0], dtype=np.int64)), dict(ao=np.array([3, 0], dtype=np.int64))):
        assert call(**bad) == -6, bad
    # the cap is 2048 tracks
    many = np.zeros(2050, dtype=np.int64)
    assert call(a=None, ao=many, t=2049) == -6 and b"n_tracks 2049 outside [0, 2048]" in L.gat_last_error(ctx._h)
    # a track must be normalized, and the message names the track and the group; a segment list need not be
    for bad in (_lib_seg([(0, 4), (3, 8), (20, 22)]), _lib_seg([(4, 8), (0, 4), (20, 22)]), _lib_seg([(0, 4), (6, 6), (20, 22)])):
        assert call(a=bad) == -6 and b"annotation track 0, group 0 is not normalized" in L.gat_last_error(ctx._h)
        assert call(lists=bad, lo=aoff) == 0
    a6, o6 = M.csr([[[(0, 4)], [], [(5, 6)]], [[(1, 2)], [(3, 4)], [(9, 12), (11, 13)]]])
    l3, lo3 = M.csr([[[(0, 4)], [(2, 3)], []]])
    out2 = np.full((1, 3), -1, dtype=np.int64)
    assert call(lists=l3, lo=lo3, a=a6, ao=o6, t=2, g=3, o=out2) == -6
    assert b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h) and out2.min() == -1
    out[:] = keep
    assert call(t=0) == 0 and call(n=0) == 0 and np.array_equal(out, keep)                  # nothing to write
    assert call() == 0 and np.array_equal(out, keep)                                           # the context is still good


def _lib_seg(pairs):
    return M.csr([[pairs]])[0]


# ---- 2. gat_sample_pair_enrichment ----------------------------------------------------------------------------------------------------
SEED, SAMPLES = 77, 48
PROBLEMS = ("annotator-units", "segments-units", "shift-units", "global-permutation-units", "local-permutation-units", "brute-force-units",
            "segments-genome", "annotator-genome-isochores") + CC.CIRCULAR_NAMES
SAMPLE_TRACKS = (3, 66)


def tracks_for(flat, T, seed=5):
    """T tracks over the contigs of a problem, of 1 to 70 intervals a contig; the second is empty on the last contig"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = []
    for t in range(T):
        k, max_len = ((60, 0), (12, 9), (70, 40), (1, 0), (5, 200))[t % 5]
        per = []
        for c in range(len(ext)):
            span = max(50, int(ext[c]))
            per.append([(a, b) for a, b in M.random_normalized(r, k, span, max_len or max(2, span // 40)) if b < 2 ** 32])
        tracks.append(per)
    if T > 1:
        tracks[1][len(ext) - 1] = []
    return tracks


def observed_for(values):
    """an obs per pair that meets every branch: the median of the pair's sample values (n_eq > 0), 0 for every third pair, and
    max + 1 for every fifth"""
    obs = np.sort(values, axis=0)[len(values) // 2].copy()
    obs[::3] = 0
    obs[1::5] = values.max(axis=0)[1::5] + 1
    return obs


@pytest.fixture(scope="module")
def sampled(ctx):
    """per problem: the flat problem, Problem.sample of (SEED, 0, SAMPLES) -- drawn once --, and per T the tracks and the model's
    counts [samples][P] of those lists"""
    cache = {}

    def get(name, T=None):
        if name not in cache:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            try:
                seg, off = P.sample(SEED, 0, SAMPLES)
                n_contigs = P.n_contigs
            finally:
                P.close()
            cache[name] = dict(flat=flat, seg=seg, off=off, n_contigs=n_contigs, values={})
        e = cache[name]
        if T is not None and T not in e["values"]:
            tracks = tracks_for(e["flat"], T)
            e["values"][T] = (tracks, M.from_sample(e["seg"], e["off"], e["n_contigs"], tracks))
        return e
    return get


def same_words(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=1))
    assert len(bad) == 0, (what, bad[0].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist(), len(bad))


@pytest.mark.parametrize("T", SAMPLE_TRACKS)
@pytest.mark.parametrize("name", PROBLEMS)
def test_samplers(ctx, sampled, monkeypatch, name, T):
    e = sampled(name, T)
    tracks, values = e["values"][T]
    obs = observed_for(values)
    want = M.words(values, obs)
    annos, anno_off = M.csr(tracks)
    P = _lib.Problem(ctx, e["flat"])
    try:
        for run in RUNS:                                # one batch: runs of 1, of 5 (the last one short), and the launch's own
            set_options(ctx, monkeypatch, GAT_PAIRS_SAMPLES_PER_BLOCK=run)
            got = P.sample_pair_enrichment(SEED, 0, SAMPLES, annos, anno_off, T, obs)
            same_words(got, want, (name, T, run))
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "20000")                 # a scratch budget of a few samples: several batches
    P = _lib.Problem(ctx, e["flat"])
    try:
        got = P.sample_pair_enrichment(SEED, 0, SAMPLES, annos, anno_off, T, obs)
        assert P.last_stats["n_batches"] >= 2, P.last_stats["n_batches"]
        same_words(got, want, (name, T, "batches"))
        # not vacuous: every branch of the comparison with obs
        n_less, n_eq = got[:, 3], got[:, 4]
        assert ((n_less > 0) & (n_less < SAMPLES)).any() and ((n_eq > 0) & (n_eq < SAMPLES)).any()
        assert (n_less == SAMPLES).any() and (n_less + n_eq <= SAMPLES).all() and got[:, 1].sum() == values.sum() > 0
    finally:
        P.close()
    if name == "segments-genome":              # SamplerSegments without isochore keys: lists neither sorted nor disjoint, and taken
        assert not all(M.is_normalized(e["seg"][e["off"][l]:e["off"][l + 1]]) for l in range(len(e["off"]) - 1))


# ---- 3. additivity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SAMPLE_TRACKS)
def test_additive_over_the_range(ctx, sampled, monkeypatch, T):
    """[0, k) plus [k, S) is [0, S), for k in the middle of a batch"""
    e = sampled("annotator-genome-isochores", T)
    tracks, values = e["values"][T]
    obs = observed_for(values)
    annos, anno_off = M.csr(tracks)
    P = _lib.Problem(ctx, e["flat"])
    try:
        for shift in range(16):                         # a scratch budget that takes the range in 2 to 16 batches of 3 samples and more
            monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", str(20000 << shift))
            whole = P.sample_pair_enrichment(SEED, 0, SAMPLES, annos, anno_off, T, obs)
            n_batches = P.last_stats["n_batches"]
            if n_batches <= SAMPLES // 3:
                break
        sizes = [b for b in range(1, SAMPLES + 1) if -(-SAMPLES // b) == n_batches]      # what a batch may hold, given their number
        assert n_batches >= 2 and sizes and min(sizes) >= 3, (n_batches, sizes)
        k = [k for k in range(1, SAMPLES) if all(k % b for b in sizes)][len(sizes) // 2]
        first = P.sample_pair_enrichment(SEED, 0, k, annos, anno_off, T, obs)
        rest = P.sample_pair_enrichment(SEED, k, SAMPLES, annos, anno_off, T, obs)
    finally:
        P.close()
    same_words(whole, M.words(values, obs), "whole")
    same_words(first, M.words(values[:k], obs), "[0, %d)" % k)
    assert np.array_equal(first + rest, whole)


# ---- 4. the diagonal against the count stage ------------------------------------------------------------------------------------------
def test_diagonal_is_segment_overlap(ctx):
    """pair (t, t) counts the segments that hit track t: on normalized lists that is CounterSegmentOverlap, which the count stage
    gives per sample for the problem's own annotation tracks"""
    from gat_amd import problem, synthetic
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], None)
    # the tracks as the problem holds them: cut to the workspace, contig level, track-major -- the layout the call takes
    annos, anno_off, T, S = flat["annos"], flat["anno_off"], int(flat["n_tracks"]), 40
    assert T >= 3 and len(anno_off) == T * int(flat["n_contigs"]) + 1
    assert all(M.is_normalized(annos[anno_off[l]:anno_off[l + 1]]) for l in range(len(anno_off) - 1))
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(SEED, 0, S)
        assert all(M.is_normalized(seg[off[l]:off[l + 1]]) for l in range(len(off) - 1))
        counts = P.sample_and_count(["segment-overlap"], SEED, 0, S)[0]
        assert counts.shape == (T, S) and counts.sum() > 0
        got = P.sample_pair_enrichment(SEED, 0, S, annos, anno_off, T, np.zeros(T * (T + 1) // 2, dtype=np.int64))
    finally:
        P.close()
    for t in range(T):
        k = pair_of(t, t, T)
        assert got[k, 1] == counts[t].sum() and got[k, 0] == (counts[t] > 0).sum() and got[k, 2] == (counts[t] * counts[t]).sum()


# ---- 5. error paths -------------------------------------------------------------------------------------------------------------------
def test_sample_arguments(ctx, sampled):
    L = _lib.lib()
    p = _lib._p
    T = 3
    e = sampled("annotator-units", T)
    tracks, values = e["values"][T]
    annos, anno_off = M.csr(tracks)
    obs = observed_for(values)
    P = _lib.Problem(ctx, e["flat"])
    try:
        C_ = P.n_contigs
        out = np.full((6, WORDS), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, a=annos, ao=anno_off, t=T, ob=obs, o=out):
            return L.gat_sample_pair_enrichment(c, prob, SEED, begin, end, p(a), p(ao), t, p(ob), p(o), None)

        assert call() == 0
        same_words(out, M.words(values[:2], obs), "two samples")
        keep = out.copy()
        down = anno_off.copy()
        down[1] = down[2] + 1
        negative = obs.copy()
        negative[4] = -1
        for bad in (dict(c=None), dict(prob=None), dict(ao=None), dict(ob=None), dict(o=None), dict(a=None), dict(begin=3, end=2), dict(t=-1),
                    dict(ao=down), dict(ob=negative), dict(t=2049, ao=np.zeros(2049 * C_ + 1, dtype=np.int64))):
            assert call(**bad) == -6, bad
        assert b"obs[4] = -1 is negative" in (call(ob=negative), L.gat_last_error(ctx._h))[1]
        assert b"outside [0, 2048]" in (call(t=2049, ao=np.zeros(2049 * C_ + 1, dtype=np.int64)), L.gat_last_error(ctx._h))[1]
        # sumsq must fit: n_max^2 * samples < 2^64, n_max the segments a sample can hold
        n_max = P.info()["slab_segments_per_sample"]
        too_many = -(-2 ** 64 // (n_max * n_max))
        assert call(end=too_many) == -6 and b"sumsq" in L.gat_last_error(ctx._h)
        # an unnormalized track is named: track 1, the problem's contig 2
        bad_annos = annos.copy()
        at = int(anno_off[1 * C_ + 2])
        assert anno_off[1 * C_ + 2 + 1] - at >= 2
        bad_annos["start"][at + 1] = bad_annos["end"][at] - 1
        assert call(a=bad_annos) == -6 and b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h)
        assert np.array_equal(out, keep)                                                   # no refused call wrote anything
        assert call(t=0, ao=np.zeros(1, dtype=np.int64), ob=None, o=None) == 0             # no track: nothing to write
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == 0                   # an empty range writes zeros
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], SEED, 0, 2, dev)
            assert call() == -6 and b"in flight" in L.gat_last_error(ctx._h)
            P.wait()
        finally:
            ctx.free(dev)
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        annos, anno_off = M.csr([[[(1, 2)] for _ in range(P.n_contigs)]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_pair_enrichment(1, 0, 1, annos, anno_off, 1, np.zeros(1, dtype=np.int64))
    finally:
        P.close()


# ---- 6. the script --------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES = 11, 30


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--order=track", "--include-single"],
                                   ["--with-segment-tracks", "--qvalue-method=holm", "--order=pvalue"], ["--sampler=circular"]],
                         ids=["isochores-single", "tracks", "circular"])
def test_script(ctx, tmp_path, extra):
    """the printed table is the one built here: Problem.sample of the same inputs and seeds, the model's counts and words"""
    from gat_amd import pairs, problem
    from test_pairs_host import script
    mod = script()
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--verbose=0"] + extra
    assert mod.main(["gat-pairs.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    opts, _ = mod.buildParser().parse_args(argv)
    segments, annotations, workspace = pairs.build_inputs(opts)
    names = list(annotations.tracks)
    assert len(names) >= 2
    results = []
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, wa = pairs.flatten(segments[track], workspace, pairs.make_sampler(opts))
        contigs = list(flat["contig_names"])
        csegs = problem.from_isochores(sa)
        tracks = []
        for t in names:
            per = problem.from_isochores(annotations[t].asArrays())
            tracks.append([per[c] if c in per else [] for c in contigs])
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        obs = M.all_counts([[csegs.get(c, []) for c in contigs]], tracks)[0]
        words = M.words(M.from_sample(seg, off, len(contigs), tracks), obs)
        results.extend(pairs.rows(track, names, obs, words, CLI_SAMPLES, include_single=opts.include_single))
    pairs.set_qvalues(results, opts.qvalue_method)
    sink = io.StringIO()
    pairs.write_results(sink, results, opts.output_order)
    got = "".join(l for l in open(str(tmp_path / "got.tsv")) if not l.startswith("#"))
    assert got == sink.getvalue()
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    assert len(rows) >= 1 and all(len(r) == 13 for r in rows)
    assert any(r[1] != r[2] and int(r[3]) > 0 and float(r[4]) > 0 for r in rows)
    assert any(r[1] == r[2] for r in rows) == bool(opts.include_single)
