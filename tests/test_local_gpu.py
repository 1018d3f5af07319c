"""GPU: k_local.  gat_list_bin_overlaps against the model (tests/local_model.py) on hand-made geometry at three window sizes and
two staging limits, gat_sample_bin_enrichment against the model applied to Problem.sample of the SAME problem, seed and sample
range, and scripts/gat-local.py against the table built here from Problem.sample and the model.  Every comparison is exact:
integers, or the text of a table."""
import io
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import local_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
WINDOWS = ("default", "4", "64")        # GAT_LOCAL_WINDOW_BINS
PIECES = ("default", "4")               # GAT_LOCAL_LDS_PIECES: a window's slice of 5 intervals and more ends in global memory at 4
TOP = 2 ** 32 - 1


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


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


def device_values(ctx, lists, tracks, bin_size, n_bins):
    a, a_off = csr(lists)
    b, b_off = csr(tracks)
    got, bin_off = ctx.list_bin_overlaps(a, a_off, len(lists), b, b_off, len(tracks), len(n_bins), bin_size, n_bins)
    assert bin_off.tolist() == np.concatenate([[0], np.cumsum(n_bins)]).tolist()
    return got


# ---- 1. gat_list_bin_overlaps ---------------------------------------------------------------------------------------------------------
def hand_geometry():
    """(name, lists[l][g], tracks[t][g], bin_size, n_bins[g]): at most 3 groups, 3 tracks, 64 intervals a list"""
    tens = dict(
        # group 0: 30 bins of 10 bases; group 1: no bins; group 2: 5 bins, and lists / tracks that lie beyond them
        tracks=[
            # a piece ending exactly on a bin edge, bookended intervals, an interval over 17 bins (five windows of 4)
            [[(5, 10), (10, 12), (19, 40), (95, 260)], [(0, 50)], [(60, 90)]],
            [[], [], []],                                                                      # an empty track
            [[(7 * i, 7 * i + 3) for i in range(40)], [], [(0, 50)]],                        # longer than a staging limit of 4
        ],
        lists=[
            [[(0, 10), (10, 20), (20, 21)], [(3, 9)], [(10, 20)]],                           # bookended segments
            [[(0, 300)], [], [(45, 80)]],                                                     # a segment over every window; partly beyond
            [[], [], []],                                                                      # an empty list
            [[(7, 8)], [(0, 1)], [(49, 50)]],                                                 # one base
            [[(4 * i, 4 * i + 2) for i in range(64)], [], [(55, 70)]],                       # 64 segments; wholly beyond the last bin
            [[(90, 270)], [], [(0, 50)]],
        ])
    cases = [("tens", tens["lists"], tens["tracks"], 10, [30, 0, 5]),
             ("whole-window", [[[(0, 300)]], [[(40, 80)]]], [[[(0, 300)]], [[(39, 81)]]], 10, [30])]
    r = random.Random(17)
    ones_l = [[M.random_normalized(r, n, 150, 9)] for n in (3, 20, 64)]
    ones_t = [[M.random_normalized(r, n, 150, 9)] for n in (5, 40)]
    cases.append(("one-base-bins", ones_l, ones_t, 1, [130]))
    odd_l = [[M.random_normalized(r, 64, 9000, 300), M.random_normalized(r, 10, 9000, 900)] for _ in range(3)]
    odd_t = [[M.random_normalized(r, 60, 9000, 200), M.random_normalized(r, 3, 9000, 2000)] for _ in range(2)]
    cases.append(("sevens", odd_l, odd_t, 7, [1000, 1290]))
    # coordinates up to 2^32 - 1 in bins of 2^31; a third bin no coordinate reaches
    far_l = [[[(5, TOP)], [(2 ** 31 - 3, 2 ** 31 + 3)]], [[(2 ** 31, TOP)], []]]
    far_t = [[[(2 ** 31 - 1, 2 ** 31 + 1), (TOP - 1, TOP)], [(0, TOP)]], [[(0, 1), (TOP - 7, TOP)], [(2 ** 31, 2 ** 31 + 1)]]]
    cases.append(("far", far_l, far_t, 2 ** 31, [2, 3]))
    return cases


def test_hand_geometry_is_what_it_says():
    name, lists, tracks, bin_size, n_bins = hand_geometry()[0]
    want = M.all_values(lists, tracks, bin_size, n_bins)
    assert want[0, 0, :3].tolist() == [5, 3, 1] and want[1, 0, 9:26].tolist() == [5] + [10] * 15 + [10]       # bins covered whole
    assert want[:, 1].sum() == 0 and want[2].sum() == 0 and want[4, :, 30:].sum() == 0 and want[1, 2, 34] == 5
    far = hand_geometry()[-1]
    assert M.all_values(*far[1:])[0, 0].tolist() == [1, 2, 3, 3, 0]


@pytest.mark.parametrize("case", hand_geometry(), ids=lambda c: c[0])
def test_list_bin_overlaps(ctx, monkeypatch, case):
    """the model's values, whatever the window and the staging limit"""
    name, lists, tracks, bin_size, n_bins = case
    for l in lists:
        assert len(l) <= 3 and all(len(x) <= 64 and M.is_normalized(x) for x in l)
    want = M.all_values(lists, tracks, bin_size, n_bins)
    assert want.sum() > 0
    for window in WINDOWS:
        for pieces in PIECES:
            for key, value in (("GAT_LOCAL_WINDOW_BINS", window), ("GAT_LOCAL_LDS_PIECES", pieces)):
                if value != "default":
                    monkeypatch.setitem(ctx.options, key, value)
                else:
                    monkeypatch.delitem(ctx.options, key, raising=False)
            got = device_values(ctx, lists, tracks, bin_size, n_bins)
            assert got.dtype == np.int64 and got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (name, window, pieces, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, annos = seg_array([(1, 5), (30, 40)]), seg_array([(0, 4), (4, 8), (20, 32)])
    off, aoff, boff = np.array([0, 2], dtype=np.int64), np.array([0, 3], dtype=np.int64), np.array([0, 5], dtype=np.int64)
    out = np.full((1, 1, 5), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, a=annos, ao=aoff, t=1, g=1, b=10, bo=boff, o=out):
        return L.gat_list_bin_overlaps(c, p(lists), p(lo), n, p(a), p(ao), t, g, b, p(bo), p(o))

    assert call() == 0 and out[0, 0].tolist() == [4, 0, 0, 2, 0]
    keep = out.copy()
    for bad in (dict(c=None), dict(lo=None), dict(ao=None), dict(bo=None), dict(o=None), dict(lists=None), dict(a=None), dict(n=-1),
                dict(t=-1), dict(g=-1), dict(lo=np.array([2, 0], dtype=np.int64)), dict(ao=np.array([3, 0], dtype=np.int64)),
                dict(b=0), dict(b=-5), dict(b=2 ** 31 + 1), dict(bo=np.array([5, 0], dtype=np.int64)), dict(bo=np.array([-1, 4], dtype=np.int64))):
        assert call(**bad) == -6, bad
    assert b"bin_size 0 outside" in (call(b=0), L.gat_last_error(ctx._h))[1]
    assert b"bin_off decreases" in (call(bo=np.array([5, 0], dtype=np.int64)), L.gat_last_error(ctx._h))[1]
    # both sides must be normalized, and the message names the list or track and the group
    for bad in (seg_array([(0, 4), (3, 8), (20, 22)]), seg_array([(4, 8), (0, 4), (20, 22)]), seg_array([(0, 4), (6, 6), (20, 22)])):
        assert call(a=bad) == -6 and b"annotation track 0, group 0 is not normalized" in L.gat_last_error(ctx._h)
        assert call(lists=bad, lo=aoff) == -6 and b"segment list 0, group 0 is not normalized" in L.gat_last_error(ctx._h)
    a6, o6 = csr([[[(0, 4)], [], [(5, 6)]], [[(1, 2)], [(3, 4)], [(9, 12), (11, 13)]]])
    l3, lo3 = csr([[[(0, 4)], [(2, 3)], []]])
    out2 = np.full((1, 2, 6), -1, dtype=np.int64)
    assert call(lists=l3, lo=lo3, a=a6, ao=o6, t=2, g=3, bo=np.array([0, 2, 4, 6], dtype=np.int64), o=out2) == -6
    assert b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h) and out2.min() == -1
    assert np.array_equal(out, keep)
    # bin_size 2^31 is the largest
    assert call(b=2 ** 31, bo=np.array([0, 1], dtype=np.int64)) == 0 and out[0, 0, 0] == 6


# ---- 2. gat_sample_bin_enrichment -----------------------------------------------------------------------------------------------------
SEED, SAMPLES = 77, 12
PROBLEMS = ("annotator-units", "shift-units", "global-permutation-units", "local-permutation-units", "brute-force-units",
            "annotator-genome-isochores", "segments-genome-isochores") + CC.CIRCULAR_NAMES
BIN_SIZES = (1, 64, 1000)


def tracks_for(flat, seed=5):
    """three tracks over the contigs of a problem: one that covers about half of every contig in long intervals (bins covered
    whole), a dozen short intervals, and up to 70 that leave the last contig empty"""
    r = random.Random(seed)
    ext = CC.extents(flat)
    tracks = []
    for k, max_len in ((60, 0), (12, 9), (70, 40)):
        per = []
        for c in range(len(ext)):
            span = max(50, int(ext[c]))
            t = M.random_normalized(r, k, span, max_len or max(2, span // 60))
            per.append([(a, b) for a, b in t if b < 2 ** 32])
        tracks.append(per)
    tracks[2][len(ext) - 1] = []
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
    """per problem: the flat problem, its tracks, Problem.sample of (SEED, 0, SAMPLES) -- drawn once -- and per bin size the
    model's values [samples][tracks][bins] of those lists"""
    cache = {}

    def get(name, bin_size=None):
        if name not in cache:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            try:
                seg, off = P.sample(SEED, 0, SAMPLES)
                n_contigs = P.n_contigs
            finally:
                P.close()
            cache[name] = dict(flat=flat, tracks=tracks_for(flat), seg=seg, off=off, n_contigs=n_contigs, values={})
        e = cache[name]
        if bin_size is not None and bin_size not in e["values"]:
            n_bins = CC.bins_for(e["flat"], bin_size)
            e["values"][bin_size] = (n_bins, M.from_sample(e["seg"], e["off"], e["n_contigs"], e["tracks"], bin_size, n_bins))
        return e
    return get


def same_words(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


@pytest.mark.parametrize("bin_size", BIN_SIZES)
@pytest.mark.parametrize("name", PROBLEMS)
def test_samplers(ctx, sampled, name, bin_size):
    e = sampled(name, bin_size)
    n_bins, values = e["values"][bin_size]
    assert all(M.is_normalized(e["seg"][e["off"][l]:e["off"][l + 1]]) for l in range(len(e["off"]) - 1))
    obs = observed_for(values)
    want = M.words(values, obs)
    annos, anno_off = csr(e["tracks"])
    P = _lib.Problem(ctx, e["flat"])
    try:
        got, bin_off = P.sample_bin_enrichment(SEED, 0, SAMPLES, annos, anno_off, 3, bin_size, n_bins, obs)
        assert got.shape == (3, int(n_bins.sum()), 5) and bin_off[-1] == n_bins.sum()
        same_words(got, want, (name, bin_size))
        # not vacuous: a bin some but not all samples reach, one where the observed value is met, one where it lies inside the null
        n_pos, n_less, n_eq = got[..., 0], got[..., 3], got[..., 4]
        assert ((n_pos > 0) & (n_pos < SAMPLES)).any() and ((n_eq > 0) & (obs > 0)).any() and ((n_less > 0) & (n_less < SAMPLES)).any()
        assert (n_less + n_eq <= SAMPLES).all() and got[..., 1].sum() == values.sum()
        # split invariance: [0, 12) is [0, 5) and [5, 12)
        a, _ = P.sample_bin_enrichment(SEED, 0, 5, annos, anno_off, 3, bin_size, n_bins, obs)
        b, _ = P.sample_bin_enrichment(SEED, 5, SAMPLES, annos, anno_off, 3, bin_size, n_bins, obs)
        same_words(a, M.words(values[:5], obs), (name, bin_size, "[0, 5)"))
        assert np.array_equal(a + b, got)
    finally:
        P.close()


@pytest.mark.parametrize("window", ["4", "64"])
@pytest.mark.parametrize("S", [1, 3, 4, 5, 9])
def test_runs_of_four_samples(ctx, sampled, monkeypatch, S, window):
    """GAT_LOCAL_SAMPLES_PER_BLOCK=4: one run that is not full, one full, one and a bit, two and a bit -- in small windows"""
    e = sampled("annotator-genome-isochores", 64)
    n_bins, values = e["values"][64]
    obs = observed_for(values)
    annos, anno_off = csr(e["tracks"])
    monkeypatch.setitem(ctx.options, "GAT_LOCAL_SAMPLES_PER_BLOCK", "4")
    monkeypatch.setitem(ctx.options, "GAT_LOCAL_WINDOW_BINS", window)
    monkeypatch.setitem(ctx.options, "GAT_LOCAL_LDS_PIECES", "4")
    P = _lib.Problem(ctx, e["flat"])
    try:
        got, _ = P.sample_bin_enrichment(SEED, 0, S, annos, anno_off, 3, 64, n_bins, obs)
    finally:
        P.close()
    same_words(got, M.words(values[:S], obs), (S, window))
    assert got[..., 0].sum() > 0


def test_many_batches(ctx, sampled, monkeypatch):
    """a scratch budget of a few samples: the range goes through in several batches, the words are those of one"""
    e = sampled("annotator-genome-isochores", 64)
    n_bins, values = e["values"][64]
    obs = observed_for(values)
    annos, anno_off = csr(e["tracks"])
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, e["flat"])
    try:
        got, _ = P.sample_bin_enrichment(SEED, 0, SAMPLES, annos, anno_off, 3, 64, n_bins, obs)
        assert P.last_stats["n_batches"] >= 2, P.last_stats["n_batches"]
    finally:
        P.close()
    same_words(got, M.words(values, obs), "batches")


def test_sample_arguments(ctx, sampled):
    L = _lib.lib()
    p = _lib._p
    e = sampled("annotator-units", 1000)
    n_bins, values = e["values"][1000]
    annos, anno_off = csr(e["tracks"])
    bin_off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int64)
    total = int(bin_off[-1])
    obs = observed_for(values)[:, :total].copy()
    P = _lib.Problem(ctx, e["flat"])
    try:
        C_ = P.n_contigs
        out = np.full((3, total, 5), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, a=annos, ao=anno_off, t=3, b=1000, bo=bin_off, ob=obs, o=out):
            return L.gat_sample_bin_enrichment(c, prob, SEED, begin, end, p(a), p(ao), t, b, p(bo), p(ob), p(o), None)

        assert call() == 0
        same_words(out, M.words(values[:2], obs), "two samples")
        keep = out.copy()
        down = anno_off.copy()
        down[1] = down[2] + 1
        bins_down = bin_off.copy()
        bins_down[1] = bins_down[2] + 1
        negative = obs.copy()
        negative[1, 3] = -1
        for bad in (dict(c=None), dict(prob=None), dict(ao=None), dict(bo=None), dict(ob=None), dict(o=None), dict(a=None),
                    dict(begin=3, end=2), dict(t=-1), dict(ao=down), dict(b=0), dict(b=2 ** 31 + 1), dict(bo=bins_down), dict(ob=negative)):
            assert call(**bad) == -6, bad
        assert b"bin_size 0 outside" in (call(b=0), L.gat_last_error(ctx._h))[1]
        assert b"bin_off decreases at group 1" in (call(bo=bins_down), L.gat_last_error(ctx._h))[1]
        assert b"negative" in (call(ob=negative), L.gat_last_error(ctx._h))[1]
        # sumsq must fit: bin_size^2 * samples < 2^64
        assert call(b=2 ** 31, end=4) == -6 and b"sumsq" in L.gat_last_error(ctx._h)
        assert call(b=2 ** 31, end=3) == 0 and call(b=2 ** 16, begin=0, end=2) == 0
        # an unnormalized track is named: track 1, the problem's contig 2
        bad_annos = annos.copy()
        at = int(anno_off[1 * C_ + 2])
        assert anno_off[1 * C_ + 2 + 1] - at >= 2
        bad_annos["start"][at + 1] = bad_annos["end"][at] - 1
        assert call(a=bad_annos) == -6 and b"annotation track 1, group 2 is not normalized at interval 1" in L.gat_last_error(ctx._h)
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == 0           # an empty range writes zeros
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


def test_unsorted_sampler_is_refused(ctx):
    """SamplerSegments without isochore keys leaves lists that are neither sorted nor disjoint: refused, and the message says so"""
    flat = CC.genome_problem(CC.SEGMENTS, False)
    tracks = tracks_for(flat)
    annos, anno_off = csr(tracks)
    n_bins = CC.bins_for(flat, 1000)
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(SEED, 0, 4)
        assert not all(M.is_normalized(seg[off[l]:off[l + 1]]) for l in range(len(off) - 1))
        with pytest.raises(ValueError, match="not normalized"):
            P.sample_bin_enrichment(SEED, 0, 4, annos, anno_off, 3, 1000, n_bins, np.zeros((3, int(n_bins.sum())), dtype=np.int64))
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
            P.sample_bin_enrichment(1, 0, 1, annos, anno_off, 1, 10, [1] * P.n_contigs, np.zeros((1, P.n_contigs), dtype=np.int64))
    finally:
        P.close()


# ---- 3. the script ------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES, CLI_BIN = 11, 30, 5000


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--order=track"],
                                   ["--with-segment-tracks", "--qvalue-method=holm"], ["--sampler=circular"]],
                         ids=["isochores", "tracks", "circular"])
def test_script(ctx, tmp_path, extra):
    """the printed table is the one built here: Problem.sample of the same inputs and seeds, the model's values and words"""
    from gat_amd import local, problem
    from test_local_host import script
    mod = script()
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--bin-size=%d" % CLI_BIN, "--verbose=0"] + extra
    assert mod.main(["gat-local.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    opts, _ = mod.buildParser().parse_args(argv)
    segments, annotations, workspace = local.build_inputs(opts)
    names = list(annotations.tracks)
    assert len(names) >= 2
    results = []
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, wa = local.flatten(segments[track], workspace, local.make_sampler(opts))
        contigs = list(flat["contig_names"])
        cws, csegs = problem.from_isochores(wa), problem.from_isochores(sa)
        n_bins = [(int(cws[c]["end"].max()) + CLI_BIN - 1) // CLI_BIN for c in contigs]
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
        obs = M.all_values([[csegs.get(c, []) for c in contigs]], tracks, CLI_BIN, n_bins)[0]
        words = M.words(M.from_sample(seg, off, len(contigs), tracks, CLI_BIN, n_bins), obs)
        results.extend(local.rows(track, names, contigs, np.concatenate([[0], np.cumsum(n_bins)]), CLI_BIN, obs, words, CLI_SAMPLES))
    local.set_qvalues(results, opts.qvalue_method)
    sink = io.StringIO()
    local.write_results(sink, results, opts.output_order)
    got = "".join(l for l in open(str(tmp_path / "got.tsv")) if not l.startswith("#"))
    assert got == sink.getvalue()
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    assert len(rows) > 20 and all(len(r) == 13 for r in rows)
    assert any(int(r[5]) > 0 and float(r[6]) > 0 for r in rows) and any(0 < int(r[12]) < CLI_SAMPLES for r in rows)
