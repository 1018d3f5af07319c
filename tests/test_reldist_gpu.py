"""GPU: k_reldist.  gat_list_reldist against the model (tests/reldist_model.py) on the hand-made geometry of
tests/reldist_cases.py, the argument errors, gat_sample_reldist_enrichment against the model applied to Problem.sample of the
SAME problem, seed and sample range, and scripts/gat-reldist.py against the table built here from Problem.sample and the model.
Every comparison is exact: integers, or the text of a table.  Every case runs at three staging limits and three runs of lists."""
import io
import itertools
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import reldist_cases as RC
import reldist_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
POINTS = ("default", "0", "4")          # GAT_RELDIST_LDS_POINTS: none staged; a (track, group) of 5 points and more ends in global memory at 4
RUNS = ("default", "1", "3")            # GAT_RELDIST_SAMPLES_PER_BLOCK
KNOBS = list(itertools.product(POINTS, RUNS))
ERR_ARG = -6


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_knobs(ctx, monkeypatch, points, run):
    for key, value in (("GAT_RELDIST_LDS_POINTS", points), ("GAT_RELDIST_SAMPLES_PER_BLOCK", run)):
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


# ---- 1. gat_list_reldist --------------------------------------------------------------------------------------------------------------
CASES = [(name, lists, points, B) for name, lists, points, bins in RC.hand_geometry() for B in bins]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-B%d" % (c[0], c[3]))
def test_list_reldist(ctx, monkeypatch, case):
    """the model's values, whatever the staging limit and the run"""
    name, lists, points, B = case
    assert len(lists) <= 6 and len(points) <= 3 and all(len(l) <= 3 for l in lists)
    want = M.values(lists, points, B)
    assert want.sum() > 0
    a, a_off = csr(lists)
    pos, off = M.point_arrays(points)
    for k_points, run in KNOBS:
        set_knobs(ctx, monkeypatch, k_points, run)
        got = ctx.list_reldist(a, a_off, len(lists), pos, off, len(points), len(points[0]), B)
        assert got.dtype == np.int64 and got.shape == want.shape == (len(lists), len(points), B + 3)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, B, k_points, run, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ---- 2. the argument errors -----------------------------------------------------------------------------------------------------------
def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, off = seg_array([(138, 143), (150, 151), (200, 201)]), np.array([0, 3], dtype=np.int64)
    pos, poff = np.array([100, 200], dtype=np.uint32), np.array([0, 2], dtype=np.int64)
    out = np.full((1, 1, 13), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, ps=pos, po=poff, t=1, g=1, b=10, o=out):
        return L.gat_list_reldist(c, p(lists), p(lo), n, p(ps), p(po), t, g, b, p(o))

    def message(**bad):
        assert call(**bad) == ERR_ARG, bad
        return L.gat_last_error(ctx._h)

    # bins 8 and 9, n = 2: C = 0 .. 0, 1, 2; D = 2 (1 + .. + 8) + |10 - 18| + |20 - 20| = 80 of n B B = 200
    assert call() == 0 and out[0, 0].tolist() == [0] * 8 + [1, 1, 400000, 2, 1]
    keep = out.copy()
    for bad in (dict(c=None), dict(lo=None), dict(po=None), dict(o=None), dict(lists=None), dict(ps=None), dict(n=-1), dict(t=-1),
                dict(g=-1), dict(lo=np.array([3, 0], dtype=np.int64)), dict(po=np.array([2, 0], dtype=np.int64)), dict(b=0), dict(b=-1),
                dict(b=1025)):
        assert call(**bad) == ERR_ARG, bad
    assert b"n_bins 0 outside" in message(b=0) and b"n_bins 1025 outside" in message(b=1025) and b"NULL" in message(ps=None)
    assert b"list_off decreases" in message(lo=np.array([3, 0], dtype=np.int64)) and b"point_off decreases" in message(po=np.array([2, 0], dtype=np.int64))
    assert b"n_lists -1" in message(n=-1) and b"n_tracks -1" in message(t=-1)
    # the points of a (track, group) ascend strictly -- named by track and group
    p3 = np.array([7, 100, 101, 50, 60], dtype=np.uint32)
    o3 = np.array([0, 1, 1, 3, 3, 5, 5], dtype=np.int64)          # 2 tracks x 3 groups: (0,0) 1, (0,2) 2, (1,1) 2
    l3, lo3 = csr([[[(0, 4)], [(52, 53)], [(100, 101)]]])
    out3 = np.full((1, 2, 5), -1, dtype=np.int64)
    three = dict(lists=l3, lo=lo3, po=o3, t=2, g=3, b=2, o=out3)
    # either track: one segment inside, in bin 0 of 2 (D = |2 - 1| + |2 - 2| = 1 of n B B = 4), and two on groups without two points
    assert call(ps=p3, **three) == 0 and out3[0].tolist() == [[1, 0, 250000, 1, 2], [1, 0, 250000, 1, 2]]
    assert b"point track 0, group 2 is not strictly ascending at point 1" in message(ps=np.array([7, 100, 100, 50, 60], dtype=np.uint32), **three)
    assert b"point track 1, group 1 is not strictly ascending at point 1" in message(ps=np.array([7, 100, 101, 60, 50], dtype=np.uint32), **three)
    assert np.array_equal(out, keep) and out3[0].tolist() == [[1, 0, 250000, 1, 2], [1, 0, 250000, 1, 2]]
    # B = 1024 at the top: the largest output row
    big = np.full((1, 1, 1027), -1, dtype=np.int64)
    assert call(b=1024, o=big) == 0 and big[0, 0, 1024:].tolist() == [M.area_of(big[0, 0, :1024].tolist()), 2, 1] and big[0, 0, :1024].sum() == 2
    # nothing to do: nothing is written; lists and points may be NULL where they hold nothing
    out[:] = -1
    assert call(n=0, lo=np.array([0], dtype=np.int64)) == 0 and call(t=0, po=np.array([0], dtype=np.int64)) == 0 and out.min() == out.max() == -1
    assert call(lists=None, lo=np.array([0, 0], dtype=np.int64)) == 0 and out[0, 0].tolist() == [0] * 13
    assert call(ps=None, po=np.array([0, 0], dtype=np.int64)) == 0 and out[0, 0].tolist() == [0] * 12 + [3]


# ---- 3. gat_sample_reldist_enrichment ---------------------------------------------------------------------------------------------------
SEED, SAMPLES, FEW, SPLIT = 77, 40, 7, 5
PROBLEMS = tuple(CC.SIX)
assert set(CC.CIRCULAR_NAMES) <= set(PROBLEMS) and "segments-genome" in PROBLEMS      # plain SamplerSegments included
BINS = (50, 3)


def points_for(flat, seed=5):
    """three tracks of points inside the workspace of every contig: 17 and more a contig, three a contig at the quarters -- what
    lies in the first and the last quarter is outside --, and six on the longest contig alone"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = [[], [], []]
    for c in range(len(ext)):
        span = max(60, int(ext[c]))
        tracks[0].append(RC.spread_points(r, min(19, span // 3), span))
        tracks[1].append([span * (k + 1) // 4 for k in range(3)])
        tracks[2].append([span * (k + 1) // 8 for k in range(6)] if c == int(np.argmax(ext)) else [])
    return tracks


def observed_for(values):
    """an obs per (track, value) that meets the null where it can: the value of sample 1, that value + 1 at every third index, 0
    at every fifth"""
    obs = values[1].copy()
    obs[:, ::3] += 1
    obs[:, ::5] = 0
    return obs


@pytest.fixture(scope="module")
def sampled(ctx):
    """per problem: the flat problem, its points, Problem.sample of (SEED, 0, SAMPLES) -- drawn once -- and per B the model's
    values [samples][tracks][B + 3] of those lists"""
    cache = {}

    def get(name, B=None):
        if name not in cache:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            try:
                seg, off = P.sample(SEED, 0, SAMPLES)
                n_contigs = P.n_contigs
            finally:
                P.close()
            cache[name] = dict(flat=flat, points=points_for(flat), seg=seg, off=off, n_contigs=n_contigs, values={})
        e = cache[name]
        if B is not None and B not in e["values"]:
            e["values"][B] = M.from_sample(e["seg"], e["off"], e["n_contigs"], e["points"], B)
        return e
    return get


def same_words(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


@pytest.mark.parametrize("B", BINS, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("name", PROBLEMS)
def test_samplers(ctx, sampled, monkeypatch, name, B):
    e = sampled(name, B)
    values = e["values"][B]
    assert values.shape == (SAMPLES, 3, B + 3)
    obs = observed_for(values)
    want = M.words(values, obs)
    # not vacuous, by the model alone: every track has a sample with a segment inside, some bin's observed value lies inside the
    # null, and the area is above 0 in some sample
    assert (values[..., B + 1] > 0).any(axis=0).all()
    assert ((want[:, :B, 3] > 0) & (want[:, :B, 3] < SAMPLES)).any() and (want[:, B, 0] > 0).all()
    pos, off = M.point_arrays(e["points"])
    P = _lib.Problem(ctx, e["flat"])
    try:
        for k_points, run in KNOBS:
            set_knobs(ctx, monkeypatch, k_points, run)
            what = (name, B, k_points, run)
            got = P.sample_reldist_enrichment(SEED, 0, SAMPLES, pos, off, 3, B, obs)
            same_words(got, want, what)
            few = P.sample_reldist_enrichment(SEED, 0, FEW, pos, off, 3, B, obs)
            same_words(few, M.words(values[:FEW], obs), what + ("[0, 7)",))
            # a range that does not start at 0, and split additivity: [0, 40) is [0, 5) and [5, 40)
            a = P.sample_reldist_enrichment(SEED, 0, SPLIT, pos, off, 3, B, obs)
            b = P.sample_reldist_enrichment(SEED, SPLIT, SAMPLES, pos, off, 3, B, obs)
            same_words(b, M.words(values[SPLIT:], obs), what + ("[5, 40)",))
            assert np.array_equal(a + b, got)
    finally:
        P.close()


def test_outside_is_reached(sampled):
    """on some problem (on every one where segments fall into the outer quarters of a contig) the model counts segments outside"""
    B = BINS[0]
    reached = [name for name in PROBLEMS if (sampled(name, B)["values"][B][..., B + 2] > 0).any()]
    assert reached, "no problem has a segment outside the points"


def test_unsorted_lists_are_taken(sampled):
    """SamplerSegments without isochore keys leaves lists that are neither sorted nor disjoint: test_samplers runs on them"""
    e = sampled("segments-genome")
    from local_model import is_normalized
    assert not all(is_normalized(e["seg"][e["off"][l]:e["off"][l + 1]]) for l in range(len(e["off"]) - 1))


def test_many_batches(ctx, sampled, monkeypatch):
    """a scratch budget of a few samples: the range goes through in several batches, the words are those of one"""
    B = BINS[0]
    e = sampled("annotator-genome-isochores", B)
    values = e["values"][B]
    obs = observed_for(values)
    pos, off = M.point_arrays(e["points"])
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, e["flat"])
    try:
        got = P.sample_reldist_enrichment(SEED, 0, SAMPLES, pos, off, 3, B, obs)
        assert P.last_stats["n_batches"] >= 2, P.last_stats["n_batches"]
    finally:
        P.close()
    same_words(got, M.words(values, obs), "batches")


def test_sample_arguments(ctx, sampled):
    L = _lib.lib()
    p = _lib._p
    B = BINS[0]
    e = sampled("annotator-units", B)
    values = e["values"][B]
    pos, off = M.point_arrays(e["points"])
    obs = observed_for(values)
    P = _lib.Problem(ctx, e["flat"])
    try:
        C_ = P.n_contigs
        out = np.full((3, B + 3, 5), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, ps=pos, po=off, t=3, b=B, ob=obs, o=out):
            return L.gat_sample_reldist_enrichment(c, prob, SEED, begin, end, p(ps), p(po), t, b, p(ob), p(o), None)

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
        for bad in (dict(c=None), dict(prob=None), dict(po=None), dict(ob=None), dict(o=None), dict(ps=None), dict(begin=3, end=2),
                    dict(t=-1), dict(po=down), dict(b=0), dict(b=1025), dict(ob=negative)):
            assert call(**bad) == ERR_ARG, bad
        assert b"n_bins 0 outside" in message(b=0) and b"negative" in message(ob=negative) and b"sample_end < sample_begin" in message(begin=3, end=2)
        assert b"point_off decreases" in message(po=down)
        # sumsq must fit: bound^2 * samples < 2^64 with bound = max(10^6, the segments a sample can hold) -- 10^6 here, and
        # 2^64 = 18 446 744.07 x 10^12: the first range that is refused (nothing runs; the one below it would sample for minutes)
        assert b"sumsq" in message(end=18446745) and b"sumsq" in message(begin=5, end=18446750)
        # points out of order are named: track 1, the problem's contig 2
        at = int(off[1 * C_ + 2])
        assert off[1 * C_ + 2 + 1] - at >= 2
        bad_pos = pos.copy()
        bad_pos[at + 1] = bad_pos[at]
        assert b"point track 1, group 2 is not strictly ascending at point 1" in message(ps=bad_pos)
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == 0           # an empty range writes zeros
        out[:] = -1
        assert call(t=0, po=np.array([0], dtype=np.int64)) == 0 and out.min() == out.max() == -1       # no track: nothing is written
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


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        pos, off = M.point_arrays([[[1, 5] for _ in range(P.n_contigs)]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_reldist_enrichment(1, 0, 1, pos, off, 1, 2, np.zeros((1, 5), dtype=np.int64))
    finally:
        P.close()


# ---- 4. the script --------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES = 11, 30


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--order=track", "--bins=7"],
                                   ["--with-segment-tracks", "--qvalue-method=holm", "--annotation-point=end", "--bins=5"],
                                   ["--annotations-label=all", "--order=annotation", "--annotation-point=start", "--bins=50"],
                                   ["--sampler=segments", "--bins=4"]],
                         ids=["isochores", "tracks-end", "pooled", "segments"])
def test_script(ctx, tmp_path, extra):
    """the printed table is the one built here: Problem.sample of the same inputs and seeds, the model's values and words"""
    from gat_amd import reldist, problem
    from test_reldist_host import script
    mod = script()
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--verbose=0"] + extra
    assert mod.main(["gat-reldist.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    opts, _ = mod.buildParser().parse_args(argv)
    B = opts.bins
    segments, annotations, workspace = reldist.build_inputs(opts)
    names = list(annotations.tracks)
    assert names == (["merged"] if opts.annotations_label else ["t0", "t1", "t2"])
    results = []
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, wa = reldist.flatten(segments[track], workspace, reldist.make_sampler(opts))
        contigs = list(flat["contig_names"])
        csegs = problem.from_isochores(sa)
        per = [problem.from_isochores(annotations[t].asArrays()) for t in names]
        points = [[reldist.points_of(a[c], opts.annotation_point).tolist() if c in a else [] for c in contigs] for a in per]
        assert all(any(len(g) >= 2 for g in t) for t in points)
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        obs = M.values([[csegs.get(c, []) for c in contigs]], points, B)[0]
        words = M.words(M.from_sample(seg, off, len(contigs), points, B), obs)
        results.extend(reldist.rows(track, names, [sum(len(g) for g in t) for t in points], B, obs, words, CLI_SAMPLES))
    reldist.set_qvalues(results, opts.qvalue_method)
    sink = io.StringIO()
    reldist.write_results(sink, results, opts.output_order)
    got = "".join(l for l in open(str(tmp_path / "got.tsv")) if not l.startswith("#"))
    assert got == sink.getvalue()
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    assert len(rows) == len(list(segments.tracks)) * len(names) * (B + 3) and all(len(r) == 14 for r in rows)
    bins = [r for r in rows if r[2].isdigit()]
    assert any(int(r[5]) > 0 and float(r[6]) > 0 and float(r[7]) > 0 for r in bins)        # (a null that varies)
    areas = [r for r in rows if r[2] == "area"]
    assert len(areas) == len(rows) // (B + 3) and all(0 < float(r[5]) <= 1 and 0 <= float(r[6]) <= 1 and int(r[12]) > 0 for r in areas)
    assert all(float(r[11]) == 1 for r in rows if r[2] in ("inside", "outside"))
