"""GPU: k_metagene.  gat_list_metagene against the model (tests/metagene_model.py) on hand-made geometry
(tests/metagene_cases.py; tests/test_metagene_model.py says on the CPU that the cases are what their names say), the argument
errors, gat_sample_metagene_enrichment against the model applied to Problem.sample of the SAME problem, seed and sample range,
and scripts/gat-metagene.py against the table built here from Problem.sample and the model.  Every comparison is exact:
integers, or the text of a table.  Every case runs at both staging limits and three runs of lists."""
import io
import itertools
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import metagene_cases as MC
import metagene_model as M
from gat_amd import _lib
from test_profile_gpu import PROBLEMS, SEED, SAMPLES, FEW, SPLIT, csr, observed_for, same_words, seg_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
FEATURES = ("default", "4")             # GAT_METAGENE_LDS_FEATURES: a (track, group) of 5 features and more ends in global memory at 4
RUNS = ("default", "1", "3")            # GAT_METAGENE_SAMPLES_PER_BLOCK
KNOBS = list(itertools.product(FEATURES, RUNS))
MODES = (M.BASES, M.MIDPOINTS)
ERR_ARG = -6


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_knobs(ctx, monkeypatch, features, run):
    for key, value in (("GAT_METAGENE_LDS_FEATURES", features), ("GAT_METAGENE_SAMPLES_PER_BLOCK", run)):
        if value != "default":
            monkeypatch.setitem(ctx.options, key, value)
        else:
            monkeypatch.delitem(ctx.options, key, raising=False)


def device_values(ctx, lists, features, Bb, Bf, w, mode):
    a, a_off = csr(lists)
    fs, fe, minus, off = M.feature_arrays(features)
    return ctx.list_metagene(a, a_off, len(lists), fs, fe, minus, off, len(features), len(features[0]), Bb, Bf, w, mode)


# ---- 1. gat_list_metagene -------------------------------------------------------------------------------------------------------------
def test_constants():
    assert (_lib.METAGENE_MAX_BINS, _lib.METAGENE_BASES, _lib.METAGENE_MIDPOINTS) == (1024, M.BASES, M.MIDPOINTS) == (1024, 0, 1)
    assert _lib.METAGENE_WORDS == _lib.NULL_WORDS and _lib.metagene_bins(10, 507) == 1024 and _lib.metagene_bins(11, 507) == 0


@pytest.mark.parametrize("mode", MODES, ids=["bases", "midpoints"])
@pytest.mark.parametrize("case", MC.hand_geometry(), ids=lambda c: c[0])
def test_list_metagene(ctx, monkeypatch, case, mode):
    """the model's values, whatever the staging limit and the run"""
    name, lists, features, geometries = case
    for Bb, Bf, w in geometries:
        want = M.all_values(lists, features, Bb, Bf, w, mode)
        assert want.sum() > 0
        for k_features, run in KNOBS:
            set_knobs(ctx, monkeypatch, k_features, run)
            got = device_values(ctx, lists, features, Bb, Bf, w, mode)
            assert got.dtype == np.int64 and got.shape == want.shape == (len(lists), len(features), 2 * Bf + Bb)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (name, (Bb, Bf, w), k_features, run, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ---- 2. the argument errors -----------------------------------------------------------------------------------------------------------
def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    u32, u8, i64 = (lambda x: np.array(x, dtype=np.uint32)), (lambda x: np.array(x, dtype=np.uint8)), (lambda x: np.array(x, dtype=np.int64))
    segs, off = seg_array([(95, 112), (130, 140)]), i64([0, 2])
    fs, fe, minus, foff = u32([100, 100]), u32([110, 110]), u8([0, 1]), i64([0, 2])
    out = np.full((1, 1, 6), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, s=fs, e=fe, mi=minus, fo=foff, t=1, g=1, bb=4, bf=1, w=10, mode=0, o=out):
        return L.gat_list_metagene(c, p(lists), p(lo), n, p(s), p(e), p(mi), p(fo), t, g, bb, bf, w, mode, p(o))

    def message(**bad):
        assert call(**bad) == ERR_ARG, bad
        return L.gat_last_error(ctx._h)

    assert call() == 0 and out[0, 0].tolist() == [7, 6, 4, 6, 4, 7]
    assert call(mode=1) == 0 and out[0, 0].tolist() == [0, 0, 1, 1, 0, 0]
    assert call() == 0
    keep = out.copy()
    big = np.zeros((1, 1, 1024), dtype=np.int64)
    for bad in (dict(c=None), dict(lo=None), dict(fo=None), dict(o=None), dict(lists=None), dict(s=None), dict(e=None), dict(mi=None), dict(n=-1),
                dict(t=-1), dict(g=-1), dict(lo=i64([2, 0])), dict(fo=i64([2, 0])), dict(bb=0), dict(bb=-3), dict(bf=-1),
                dict(bb=1000, bf=13, o=big), dict(bb=1025, bf=0, o=big), dict(w=0), dict(w=-5), dict(w=2 ** 31 + 1), dict(bf=0, w=0),
                dict(bf=3, w=2 ** 30), dict(mode=2), dict(mode=-1)):
        assert call(**bad) == ERR_ARG, bad
    assert b"body_bins 0 is less than 1" in message(bb=0) and b"flank_bins -1 is negative" in message(bf=-1)
    assert b"2 * flank_bins + body_bins = 1026 is more than 1024" in message(bb=1000, bf=13, o=big)
    assert b"flank_bin_size 0 outside [1, 2^31]" in message(w=0) and b"flank_bin_size 0 outside [1, 2^31]" in message(bf=0, w=0)
    assert b"flank_bins * flank_bin_size = 3 * 1073741824 is more than 2^31" in message(bf=3, w=2 ** 30)
    assert b"mode 2 is neither GAT_METAGENE_BASES nor GAT_METAGENE_MIDPOINTS" in message(mode=2)
    assert call(bb=1022, bf=1, w=2 ** 31, s=fs[:1], e=fe[:1], mi=minus[:1], fo=i64([0, 1]), o=big) == 0          # B = 1024 and F = 2^31 pass
    # the features of a (track, group): end > start, the strand 0 or 1, ascending by (start, end, minus), none twice -- named by
    # track and group
    s3, e3 = u32([7, 100, 100, 50, 50]), u32([9, 150, 150, 60, 70])
    o3 = i64([0, 1, 1, 3, 3, 5, 5])                                # 2 tracks x 3 groups: (0,0) 1, (0,2) 2, (1,1) 2
    l3, lo3 = csr([[[(0, 4)], [(2, 3)], []]])
    out3 = np.full((1, 2, 6), -1, dtype=np.int64)
    three = dict(lists=l3, lo=lo3, s=s3, e=e3, fo=o3, t=2, g=3, o=out3)
    assert call(mi=u8([0, 0, 1, 0, 1]), **three) == 0
    assert b"feature track 0, group 2 is out of order at feature 1 (ascending by start, then end, plus before minus)" in message(mi=u8([0, 1, 0, 0, 1]), **three)
    assert b"feature track 0, group 2 repeats a feature (start, end, strand) at feature 1" in message(mi=u8([0, 1, 1, 0, 1]), **three)
    assert b"feature track 1, group 1: feat_minus 2 at feature 1 is neither 0 nor 1" in message(mi=u8([0, 0, 1, 0, 2]), **three)
    assert b"feature track 1, group 1 is out of order at feature 1" in message(mi=u8([0, 0, 1, 0, 0]), **dict(three, e=u32([9, 150, 150, 60, 55])))
    assert b"feature track 1, group 1 is out of order at feature 1" in message(mi=u8([0, 0, 1, 0, 0]), **dict(three, s=u32([7, 100, 100, 50, 49])))
    assert b"feature track 0, group 2: feature 1 is empty (end <= start)" in message(mi=u8([0, 0, 1, 0, 1]), **dict(three, e=u32([9, 150, 100, 60, 70])))
    assert b"feature track 0, group 0: feature 0 is empty (end <= start)" in message(mi=u8([0, 0, 1, 0, 1]), **dict(three, e=u32([3, 150, 150, 60, 70])))
    # the lists must be normalized, and the message names the list and the group
    for bad in ([(0, 4), (3, 8)], [(4, 8), (0, 4)], [(0, 4), (6, 6)]):
        bl, blo = csr([[[(0, 4)], bad, []]])
        assert b"segment list 0, group 1 is not normalized" in message(mi=u8([0, 0, 1, 0, 1]), **dict(three, lists=bl, lo=blo))
    # a value is a 32-bit word: K_t * flank_bin_size < 2^32 with flanks, sum_f ceil(len_f / body_bins) < 2^32
    assert b"4294967296, do not fit 32 bits" in message(bb=1, bf=1, w=2 ** 31, o=np.zeros((1, 1, 3), dtype=np.int64))
    assert call(bb=1, bf=1, w=2 ** 31, s=fs[:1], e=fe[:1], mi=minus[:1], fo=i64([0, 1]), o=np.zeros((1, 1, 3), dtype=np.int64)) == 0
    assert call(bb=1, bf=0, w=2 ** 31, o=np.zeros((1, 1, 1), dtype=np.int64)) == 0          # (without flanks flank_bin_size bounds nothing)
    wide = dict(s=u32([0, 0]), e=u32([2 ** 32 - 1, 2 ** 32 - 1]))
    assert b"4294967296, do not fit 32 bits" in message(bb=2, bf=0, o=np.zeros((1, 1, 2), dtype=np.int64), **wide)
    assert call(bb=3, bf=0, o=np.zeros((1, 1, 3), dtype=np.int64), **wide) == 0
    assert np.array_equal(out, keep) and out3.min() >= 0
    # nothing to do: nothing is written
    out[:] = -1
    assert call(n=0, lo=i64([0])) == 0 and call(t=0, fo=i64([0])) == 0 and out.min() == out.max() == -1


# ---- 3. gat_sample_metagene_enrichment --------------------------------------------------------------------------------------------------
BODY, FLANK, WIDTH = 10, 5, 25
NB = 2 * FLANK + BODY


def features_for(flat, seed=5):
    """three tracks of features that span the workspace of every contig: 19 a contig on both strands that overlap and nest; the
    whole contig and its three thirds; and, on the longest contig alone, one feature over five short ones"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = [[], [], []]
    for c in range(len(ext)):
        span = max(400, int(ext[c]))
        tracks[0].append(MC.spread_features(r, 19, span, max(20, span // 6)))
        thirds = [(span * k // 3, span * (k + 1) // 3 - 40 * k, (+1, -1, +1)[k]) for k in range(3)]
        tracks[1].append(sorted([(0, span, -1)] + thirds, key=M.feature_key))
        tracks[2].append(sorted([(span // 8, span - span // 8, -1)] + [(span * (k + 2) // 9, span * (k + 2) // 9 + 30 + k, (-1) ** k) for k in range(5)],
                                key=M.feature_key) if c == int(np.argmax(ext)) else [])
    return tracks


@pytest.fixture(scope="module")
def sampled(ctx):
    """per problem: the flat problem, its features, Problem.sample of (SEED, 0, SAMPLES) -- drawn once -- and per mode the
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
            cache[name] = dict(flat=flat, features=features_for(flat), seg=seg, off=off, n_contigs=n_contigs, values={})
        e = cache[name]
        if mode is not None and mode not in e["values"]:
            e["values"][mode] = M.from_sample(e["seg"], e["off"], e["n_contigs"], e["features"], BODY, FLANK, WIDTH, mode)
        return e
    return get


@pytest.mark.parametrize("mode", MODES, ids=["bases", "midpoints"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_samplers(ctx, sampled, monkeypatch, name, mode):
    e = sampled(name, mode)
    values = e["values"][mode]
    assert all(M.is_normalized(e["seg"][e["off"][l]:e["off"][l + 1]]) for l in range(len(e["off"]) - 1))
    assert values.shape == (SAMPLES, 3, NB)
    for keys in ([M.feature_key(f) for f in g] for t in e["features"] for g in t):
        assert all(x < y for x, y in zip(keys, keys[1:]))
    obs = observed_for(values)
    want = M.words(values, obs)
    # not vacuous: the model's words are not all zero upstream, in the body and downstream, and some observed value lies inside the null
    for region in (want[:, :FLANK], want[:, FLANK:FLANK + BODY], want[:, FLANK + BODY:]):
        assert (region[..., :3] > 0).any()
    assert (want[..., 3] > 0).any() and (want[..., 4] > 0).any() and (want[..., 0] > 0).any(axis=1).all()
    args = M.feature_arrays(e["features"]) + (3, BODY, FLANK, WIDTH, mode, obs)
    P = _lib.Problem(ctx, e["flat"])
    try:
        for k_features, run in KNOBS:
            set_knobs(ctx, monkeypatch, k_features, run)
            what = (name, mode, k_features, run)
            got = P.sample_metagene_enrichment(SEED, 0, SAMPLES, *args)
            same_words(got, want, what)
            few = P.sample_metagene_enrichment(SEED, 0, FEW, *args)
            same_words(few, M.words(values[:FEW], obs), what + ("[0, 7)",))
            # a range that does not start at 0, and split additivity: [0, 40) is [0, 5) and [5, 40)
            a = P.sample_metagene_enrichment(SEED, 0, SPLIT, *args)
            b = P.sample_metagene_enrichment(SEED, SPLIT, SAMPLES, *args)
            same_words(b, M.words(values[SPLIT:], obs), what + ("[5, 40)",))
            assert np.array_equal(a + b, got)
        assert (got[..., 3] + got[..., 4] <= SAMPLES).all() and got[..., 1].sum() == values.sum()
    finally:
        P.close()


def test_many_batches(ctx, sampled, monkeypatch):
    """a scratch budget of a few samples: the range goes through in several batches, the words are those of one"""
    e = sampled("annotator-genome-isochores", M.BASES)
    values = e["values"][M.BASES]
    obs = observed_for(values)
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, e["flat"])
    try:
        got = P.sample_metagene_enrichment(SEED, 0, SAMPLES, *M.feature_arrays(e["features"]), 3, BODY, FLANK, WIDTH, M.BASES, obs)
        assert P.last_stats["n_batches"] >= 2, P.last_stats["n_batches"]
    finally:
        P.close()
    same_words(got, M.words(values, obs), "batches")


def test_sample_arguments(ctx, sampled):
    L = _lib.lib()
    p = _lib._p
    e = sampled("annotator-units", M.BASES)
    values = e["values"][M.BASES]
    fs, fe, minus, off = M.feature_arrays(e["features"])
    obs = observed_for(values)
    P = _lib.Problem(ctx, e["flat"])
    try:
        C_ = P.n_contigs
        out = np.full((3, NB, 5), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, s=fs, en=fe, mi=minus, fo=off, t=3, bb=BODY, bf=FLANK, w=WIDTH, mode=0, ob=obs, o=out):
            return L.gat_sample_metagene_enrichment(c, prob, SEED, begin, end, p(s), p(en), p(mi), p(fo), t, bb, bf, w, mode, p(ob), p(o), None)

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
        for bad in (dict(c=None), dict(prob=None), dict(fo=None), dict(ob=None), dict(o=None), dict(s=None), dict(en=None), dict(mi=None),
                    dict(begin=3, end=2), dict(t=-1), dict(fo=down), dict(bb=0), dict(bf=-1), dict(bb=1015), dict(w=0), dict(w=2 ** 31 + 1),
                    dict(w=2 ** 29), dict(mode=2), dict(ob=negative)):
            assert call(**bad) == ERR_ARG, bad
        assert b"flank_bin_size 0 outside" in message(w=0) and b"obs[23] = -1 is negative" in message(ob=negative) and b"body_bins 0" in message(bb=0)
        assert b"sample_end < sample_begin" in message(begin=3, end=2) and b"more than 2^31" in message(w=2 ** 29)
        # sumsq must fit: most^2 * samples < 2^64.  Track 0 holds K features: the flank bin size at which 2 samples pass
        K = int(off[C_] - off[0])
        w_big = (2 ** 32 - 1) // K
        one = dict(bb=1, bf=1, ob=np.zeros((3, 3), dtype=np.int64), o=np.zeros((3, 3, 5), dtype=np.int64))
        assert M.bounds(e["features"], 1, 1, w_big)[0] == K * w_big
        assert b"bases per bin^2 * samples" in message(w=w_big, **one) and b"sumsq" in message(w=w_big, **one) and call(w=w_big, end=1, **one) == 0
        assert b"do not fit 32 bits" in message(w=w_big + 1, end=1, **one)
        # features out of order are named: track 1, the problem's contig 2
        at = int(off[1 * C_ + 2])
        assert off[1 * C_ + 2 + 1] - at >= 2
        assert fs[at] == fs[at + 1] == 0 and fe[at] < fe[at + 1]            # (the first third and the whole contig)
        bad_fe = fe.copy()
        bad_fe[at + 1] = fe[at] - 1
        assert b"feature track 1, group 2 is out of order at feature 1" in message(en=bad_fe)
        bad_fs, bad_fe, bad_minus = fs.copy(), fe.copy(), minus.copy()
        bad_fs[at + 1], bad_fe[at + 1], bad_minus[at + 1] = fs[at], fe[at], minus[at]
        assert b"feature track 1, group 2 repeats a feature" in message(s=bad_fs, en=bad_fe, mi=bad_minus)
        bad_fe = fe.copy()
        bad_fe[at + 1] = fs[at + 1]
        assert b"feature track 1, group 2: feature 1 is empty" in message(en=bad_fe)
        bad_minus = minus.copy()
        bad_minus[at] = 3
        assert b"feature track 1, group 2: feat_minus 3" in message(mi=bad_minus)
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == 0           # an empty range writes zeros
        out[:] = -1
        assert call(t=0, fo=np.array([0], dtype=np.int64)) == 0 and out.min() == out.max() == -1       # no track: nothing is written
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], SEED, 0, 2, dev)
            assert b"a call is in flight on this problem" in message()
            P.wait()
        finally:
            ctx.free(dev)
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()


def test_unsorted_sampler_is_refused(ctx):
    """SamplerSegments without isochore keys leaves lists that are neither sorted nor disjoint: refused, and the message says so"""
    flat = CC.genome_problem(CC.SEGMENTS, False)
    P = _lib.Problem(ctx, flat)
    try:
        seg, soff = P.sample(SEED, 0, 4)
        assert not all(M.is_normalized(seg[soff[l]:soff[l + 1]]) for l in range(len(soff) - 1))
        with pytest.raises(ValueError, match="not normalized .SamplerSegments without isochore keys.*the metagene needs normalized lists"):
            P.sample_metagene_enrichment(SEED, 0, 4, *M.feature_arrays(features_for(flat)), 3, BODY, FLANK, WIDTH, 0, np.zeros((3, NB), dtype=np.int64))
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        args = M.feature_arrays([[[(1, 9, +1)] for _ in range(P.n_contigs)]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_metagene_enrichment(1, 0, 1, *args, 1, 2, 1, 10, 0, np.zeros((1, 4), dtype=np.int64))
    finally:
        P.close()


# ---- 4. the script --------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES, CLI_BODY, CLI_FLANK, CLI_WIDTH = 11, 30, 8, 3, 50     # (bins narrow enough that not every sample reaches every bin)


def feature_file(path):
    """a small stranded feature file over the contigs of tests/golden/cli: two named tracks, features that overlap and nest,
    alternative transcripts with one span, features shorter than the body bins, one just outside the workspace, and a contig the
    workspace lacks"""
    r = random.Random(2)
    lines = []
    for contig, top in (("chrA", 388000), ("chrB", 238000), ("chrC", 78000), ("chrD", 38000)):
        for k in range(8):
            s = r.randrange(12000, top - 6000)
            lines.append("%s\t%d\t%d\t%s\t0\t%s" % (contig, s, s + r.randrange(40, 2500), "genes" if k % 4 else "other", "+-"[k % 2]))
            if k == 6:
                lines.append(lines[-1].replace("\t0\t", "\t960\t"))                  # a second transcript with the same span
                lines.append("%s\t%d\t%d\tgenes\t0\t+" % (contig, s + 10, s + 15))   # nested, and shorter than the body bins
        lines.append("%s\t%d\t%d\tgenes\t0\t-" % (contig, 12000, top - 6000))        # one gene over all the others
    lines.append("chrA\t11000\t11990\tgenes\t0\t+")
    lines.append("chrNowhere\t5\t900\tgenes\t0\t-")
    path.write_text("\n".join(lines) + "\n")
    return str(path)


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--order=track"],
                                   ["--with-segment-tracks", "--qvalue-method=holm", "--profile-of=midpoints", "--min-feature-length=1"],
                                   ["--ignore-strand", "--annotations-label=all", "--order=annotation"], ["--sampler=circular", "--flank-bins=0"]],
                         ids=["isochores", "tracks-midpoints", "pooled", "circular-no-flanks"])
def test_script(ctx, tmp_path, extra):
    """the printed table is the one built here: Problem.sample of the same inputs and seeds, the model's values and words"""
    from gat_amd import metagene, problem
    from test_metagene_host import script
    mod = script()
    bed = feature_file(tmp_path / "features.bed")
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--features=%s" % bed,
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--body-bins=%d" % CLI_BODY, "--flank-bins=%d" % CLI_FLANK, "--flank-bin-size=%d" % CLI_WIDTH, "--verbose=0"] + extra
    assert mod.main(["gat-metagene.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    opts, _ = mod.buildParser().parse_args(argv)
    mode = metagene.PROFILES_OF.index(opts.profile_of)
    Bb, Bf, w = opts.body_bins, opts.flank_bins, opts.flank_bin_size
    segments, annotations, workspace = metagene.build_inputs(opts)
    read = metagene.read_features(opts.annotation_files, metagene.min_feature_length(opts), opts.ignore_strand, opts.annotations_label)
    assert list(read) == (["merged"] if opts.annotations_label else ["other", "genes"])
    results = []
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, wa = metagene.flatten(segments[track], workspace, metagene.make_sampler(opts))
        contigs = list(flat["contig_names"])
        assert "chrNowhere" not in contigs
        csegs = problem.from_isochores(sa)
        features = [[[(int(s), int(e), -1 if m else +1) for s, e, m in zip(*read[t][c])] if c in read[t] else [] for c in contigs] for t in read]
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        obs = M.all_values([[csegs.get(c, []) for c in contigs]], features, Bb, Bf, w, mode)[0]
        words = M.words(M.from_sample(seg, off, len(contigs), features, Bb, Bf, w, mode), obs)
        results.extend(metagene.rows(track, list(read), [sum(len(g) for g in t) for t in features], Bb, Bf, w, obs, words, CLI_SAMPLES))
    metagene.set_qvalues(results, opts.qvalue_method)
    sink = io.StringIO()
    metagene.write_results(sink, results, opts.output_order)
    got = "".join(l for l in open(str(tmp_path / "got.tsv")) if not l.startswith("#"))
    assert got == sink.getvalue()
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    assert len(rows) == len(list(segments.tracks)) * len(read) * (2 * Bf + Bb) and all(len(r) == 15 for r in rows)
    assert any(int(r[6]) > 0 and float(r[7]) > 0 for r in rows) and any(0 < int(r[13]) < CLI_SAMPLES for r in rows)
    assert sorted(set(r[3] for r in rows)) == (["body", "downstream", "upstream"] if Bf else ["body"])
    # the feature outside the workspace is kept, the transcripts with one span are one feature, the contig the workspace lacks
    # and the features shorter than --min-feature-length (the body bins, unless it is given) are dropped
    # (a segment track whose problem lacks a contig keeps fewer: the counts of the problem with all four contigs are the largest)
    if not opts.annotations_label and not opts.ignore_strand:
        counts = {a: max(int(r[14]) for r in rows if r[1] == a) for a in ("other", "genes")}
        assert counts == dict(other=8, genes=29 + 4 if opts.min_feature_length == 1 else 29)
