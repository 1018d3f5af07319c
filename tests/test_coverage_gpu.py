"""GPU: gat_sample_coverage (k_coverage) against the model (tests/coverage_model.py) applied to Problem.sample of the SAME
problem, seed and sample range -- lists the existing suite pins to the reference.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import coverage_cases as CC
import coverage_model as M
import sampler_edges as E
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _assert_same(got, want, what=""):
    for g, w, name in zip(got[:4], want, ("bases", "starts", "ends", "outside")):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


def _check(P, seg, off, seed, s0, s1, bin_size, n_bins, what=""):
    """sample_coverage of [s0, s1) against the model over the lists (seg, off) of the same range"""
    want = M.from_sample(seg, off, P.n_contigs, bin_size, n_bins)
    got = P.sample_coverage(seed, s0, s1, bin_size, n_bins)
    _assert_same(got, want, what)
    bin_off = got[4]
    for c in range(P.n_contigs):                        # nothing disappears
        lists = np.concatenate([seg[off[i * P.n_contigs + c]:off[i * P.n_contigs + c + 1]] for i in range(s1 - s0)])
        assert int(got[0][bin_off[c]:bin_off[c + 1]].sum()) + int(got[3][c]) == M.total_length(lists)
    return got


# ---- 1. six samplers ------------------------------------------------------------------------------------------------------
SIX_SEED, SIX_SAMPLES = 77, 12


@pytest.fixture(scope="module")
def six(ctx):
    """the problems of the six-sampler test with their lists, made at the first use and shared by the bin sizes"""
    made = {}

    def get(name):
        if name not in made:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            seg, off = P.sample(SIX_SEED, 0, SIX_SAMPLES)
            made[name] = (flat, P, seg, off)
        return made[name]

    yield get
    for _, P, _, _ in made.values():
        P.close()


@pytest.mark.parametrize("bin_size", CC.BIN_SIZES)
@pytest.mark.parametrize("name", sorted(CC.SIX))
def test_six_samplers(six, name, bin_size):
    flat, P, seg, off = six(name)
    assert len(seg) > 0
    got = _check(P, seg, off, SIX_SEED, 0, SIX_SAMPLES, bin_size, CC.bins_for(flat, bin_size), name)
    assert got[0].sum() > 0


def test_unsorted_route_is_taken(six):
    """SamplerSegments without isochore keys returns lists that are not sorted: the case the scan is for"""
    _, P, seg, off = six("segments-genome")
    assert any(np.any(np.diff(seg["start"][off[i]:off[i + 1]].astype(np.int64)) < 0) for i in range(len(off) - 1))


# ---- 2. window and chunk edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [CC.ANNOTATOR, CC.SEGMENTS])
@pytest.mark.parametrize("S", [1, 3, 4, 5, 9])
def test_window_and_chunk_edges(ctx, monkeypatch, sampler, S):
    """windows of 64 bins of one base over contigs of 0, 1, 63, 64, 65 and 129 bins, a contig whose lists lie beyond its
    bins, chunks of 4 samples"""
    monkeypatch.setitem(ctx.options, "GAT_COVERAGE_WINDOW_BINS", str(CC.WINDOW))
    monkeypatch.setitem(ctx.options, "GAT_COVERAGE_SAMPLES_PER_BLOCK", "4")
    P = _lib.Problem(ctx, E.units_flat(CC.window_units(), sampler))
    try:
        assert P.n_contigs == len(CC.WINDOW_BINS)
        seg, off = P.sample(CC.WINDOW_SEED, 0, S)
        if S == CC.WINDOW_SAMPLES:
            reach = CC.window_reach(seg, off)
            assert all(reach.values()), reach
        got = _check(P, seg, off, CC.WINDOW_SEED, 0, S, 1, np.array(CC.WINDOW_BINS, dtype=np.int64), (sampler, S))
        bin_off = got[4]
        last = P.n_contigs - 1
        assert got[0][bin_off[last]:].sum() == 0 and got[3][last] > 0 and got[3][0] > 0        # all of it `outside`
    finally:
        P.close()


# ---- 3. batches ---------------------------------------------------------------------------------------------------------------
def test_many_batches_and_split_invariance(ctx, monkeypatch):
    flat = CC.genome_problem(CC.ANNOTATOR, True)
    n_bins = CC.bins_for(flat, 64, cap=1 << 20)
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(8, 0, 24)
        whole = P.sample_coverage(8, 0, 24, 64, n_bins)
        assert P.last_stats["n_batches"] == 1
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")      # (a scratch budget of a few samples, for a problem made under it)
    P = _lib.Problem(ctx, flat)
    try:
        cut = _check(P, seg, off, 8, 0, 24, 64, n_bins)
        assert P.last_stats["n_batches"] > 3, P.last_stats["n_batches"]
        _assert_same(cut, whole[:4])
        a, b = P.sample_coverage(8, 0, 5, 64, n_bins), P.sample_coverage(8, 5, 24, 64, n_bins)
        _assert_same([x + y for x, y in zip(a[:4], b[:4])], whole[:4])
    finally:
        P.close()


def test_repeated_batch_is_not_accumulated_twice(ctx, monkeypatch):
    """GAT_TEST_SMALL_CAPS with a small scratch budget: batches overflow and are laid out again"""
    units, radius, extension = E.shift_edge_units(14)
    units += [x[1][0] for x in E.shift_fixed_units() if x[0] in ("fill_all_lanes", "near_zero")]
    flat = E.units_flat(units, E.SHIFT, radius, extension)
    n_bins = CC.bins_for(flat, 7)
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(31, 0, 12)
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "300000")
    P = _lib.Problem(ctx, flat)
    try:
        _check(P, seg, off, 31, 0, 12, 7, n_bins)
        assert P.last_stats["n_retried"] > 0 and P.last_stats["n_batches"] > 1, P.last_stats
    finally:
        P.close()


# ---- 4. beyond 32 bits ----------------------------------------------------------------------------------------------------------
def test_sums_beyond_32_bits(ctx):
    P = _lib.Problem(ctx, E.units_flat(CC.big_units(), CC.SEGMENTS))
    try:
        seg, off = P.sample(11, 0, CC.BIG_SAMPLES)
        n_bins = np.array([16], dtype=np.int64)
        want = M.from_sample(seg, off, 1, CC.BIG_BIN, n_bins)
        assert want[0].max() > 1 << 32                                   # the precondition, on the model
        _check(P, seg, off, 11, 0, CC.BIG_SAMPLES, CC.BIG_BIN, n_bins)
        _check(P, seg, off, 11, 0, CC.BIG_SAMPLES, 1 << 31, np.array([1], dtype=np.int64))
        _check(P, seg, off, 11, 0, CC.BIG_SAMPLES, CC.BIG_BIN, np.array([3], dtype=np.int64))     # `outside` beyond 2^32 too
    finally:
        P.close()


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    L = _lib.lib()
    flat = CC.unit_problem("annotator")
    P = _lib.Problem(ctx, flat)
    try:
        nc = P.n_contigs
        bin_off = np.arange(nc + 1, dtype=np.int64) * 5
        bases, starts, ends = (np.full(5 * nc, -1, dtype=np.int64) for _ in range(3))
        outside = np.full(nc, -1, dtype=np.int64)
        p = _lib._p

        def call(c=ctx._h, prob=P._h, begin=0, end=2, bin_size=100, off=bin_off, b=bases, s=starts, e=ends, o=outside):
            return L.gat_sample_coverage(c, prob, 5, begin, end, bin_size, p(off), p(b), p(s), p(e), p(o), None)

        assert call() == 0
        for bad in (dict(c=None), dict(prob=None), dict(off=None), dict(b=None), dict(o=None), dict(bin_size=0), dict(bin_size=-3),
                    dict(bin_size=(1 << 31) + 1), dict(begin=3, end=2)):
            assert call(**bad) == -6, bad
        assert call(bin_size=1 << 31) == 0 and call(bin_size=1) == 0
        down = bin_off.copy()
        down[2] = down[1] - 1
        assert call(off=down) == -6
        assert b"bin_off" in L.gat_last_error(ctx._h)
        # an empty range: zeros, whatever the buffers held
        assert call(begin=4, end=4) == 0
        assert not bases.any() and not starts.any() and not ends.any() and not outside.any()
        # starts / ends not wanted
        want = P.sample_coverage(5, 0, 2, 100, np.full(nc, 5))
        assert call(s=None, e=None) == 0 and np.array_equal(bases, want[0]) and np.array_equal(outside, want[3])
        got = P.sample_coverage(5, 0, 2, 100, np.full(nc, 5), want_starts_ends=False)
        assert got[1] is None and got[2] is None and np.array_equal(got[0], want[0])
        # a call in flight on the problem
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], 5, 0, 2, dev)
            assert call() == -6 and b"in flight" in L.gat_last_error(ctx._h)
            P.wait()
        finally:
            ctx.free(dev)
        assert call() == 0
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    """SamplerBruteForce that cannot converge (brute_force_edges: more bases to place than the workspace holds): the
    reference's ValueError, unchanged"""
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    P = _lib.Problem(ctx, BF.units_flat(case["units"], **case["params"]))
    try:
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_coverage(1, 0, 1, 10, [4])
        assert P.last_stats["n_unconverged"] == 1
    finally:
        P.close()


# ---- 6. the script -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--with-segment-tracks"], ["--isochores=%s" % os.path.join(CLI, "isochores.bed")],
                                   ["--with-segment-tracks", "--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--sampler=shift"]],
                         ids=["merged", "tracks", "isochores", "tracks-isochores-shift"])
def test_script(ctx, tmp_path, extra):
    from gat_amd import coverage
    from test_coverage_host import script
    mod = script()
    out = tmp_path / "coverage.tsv"
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--workspace=%s" % os.path.join(CLI, "workspace.bed"),
            "--num-samples=20", "--random-seed=9", "--bin-size=500", "--verbose=0"] + extra
    assert mod.main(["gat-coverage.py", "--stdout=%s" % out] + argv) == 0
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == list(coverage.HEADER)
    rows = [l.split("\t") for l in lines[1:] if not l.startswith("#")]
    notes = dict((tuple(l[2:].split("\t")[:2]), int(l.split("\t")[2])) for l in lines[1:] if l.startswith("#"))
    # the model: the same inputs, the lists of the same seed
    opts, _ = mod.buildParser().parse_args(argv)
    segments, workspace = coverage.build_inputs(opts)
    want_rows, want_notes = [], {}
    for track in segments.tracks:
        flat, sa, wa = coverage.flatten(segments[track], workspace, coverage.make_sampler(opts))
        from gat_amd import problem
        cws, csegs = problem.from_isochores(wa), problem.from_isochores(sa)
        names = list(flat["contig_names"])
        unsampled = [c for c in cws if c not in names]              # workspace without a segment of the track: its rows all the same
        n_bins = [(int(cws[c]["end"].max()) + 499) // 500 for c in names]
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(9, 0, 20)
        finally:
            P.close()
        bases, starts, ends, outside = M.from_sample(seg, off, len(names), 500, n_bins)
        bin_off = np.concatenate([[0], np.cumsum(n_bins)])
        for k, c in enumerate(names):
            wb, sb = M.coverage(cws[c], 500, n_bins[k])[0], M.coverage(csegs[c], 500, n_bins[k])[0]
            for b in range(n_bins[k]):
                v = bases[bin_off[k] + b]
                if wb[b] > 0 or v > 0:
                    want_rows.append([track, c, b * 500, (b + 1) * 500, wb[b], sb[b], v, starts[bin_off[k] + b], ends[bin_off[k] + b]])
            if outside[k]:
                want_notes[(track, c)] = int(outside[k])
        for c in unsampled:
            nb = (int(cws[c]["end"].max()) + 499) // 500
            wb = M.coverage(cws[c], 500, nb)[0]
            want_rows += [[track, c, b * 500, (b + 1) * 500, wb[b], 0, 0, 0, 0] for b in range(nb) if wb[b] > 0]
    assert len(rows) == len(want_rows) > 0
    for r, w in zip(rows, want_rows):
        assert r[:9] == [str(x) for x in w], (r, w)
        exact = w[6] / (20 * 500.0)
        assert abs(float(r[9]) - exact) <= 1e-12 * exact
    assert notes == want_notes
