"""GPU: a batch that overflows, is laid out again and repeated in mid-call, behind every list reduction but coverage (whose own
file has this test: the recipe is test_coverage_gpu.py::test_repeated_batch_is_not_accumulated_twice).  All gat_sample_* entry
points share for_each_sampler_batch, which repeats a batch whose slab had to grow: nothing of the first attempt may be seen,
summed or folded.  The lists are Problem.sample of the same problem made without the knobs; the words are the model's on
them.  Last, gat_sample_signal's own branch: its bound for lists that are not normalized depends on the regions' sizes and is
checked again behind a batch for which they grew."""
import ctypes as C

import numpy as np
import pytest

import coverage_cases as CC
import distance_model
import geneset_model
import local_model
import metrics_model
import pairs_model
import profile_model
import sampler_edges as E
import signal_model
import test_distance_gpu as TD
import test_geneset_gpu as TG
import test_local_gpu as TL
import test_metrics_gpu as TM
import test_pairs_gpu as TP
import test_profile_gpu as TPR
import test_signal_gpu as TS
from gat_amd import _lib

pytestmark = pytest.mark.gpu

SEED, S = 31, 12
ERR_ARG = -6


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def recipe(ctx):
    """coverage's recipe: the shift units that overflow under GAT_TEST_SMALL_CAPS, and their lists sampled without knobs"""
    units, radius, extension = E.shift_edge_units(14)
    units += [x[1][0] for x in E.shift_fixed_units() if x[0] in ("fill_all_lanes", "near_zero")]
    flat = E.units_flat(units, E.SHIFT, radius, extension)
    assert "GAT_TEST_SMALL_CAPS" not in ctx.options and "GAT_SLAB_BYTES" not in ctx.options
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(SEED, 0, S)
        assert P.last_stats["n_retried"] == 0
    finally:
        P.close()
    return flat, seg, off


@pytest.fixture
def small(ctx, monkeypatch, recipe):
    """the recipe's problem made under the knobs; behind the test: a batch was repeated, and there was more than one"""
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "300000")
    P = _lib.Problem(ctx, recipe[0])
    calls = []
    yield P, calls
    try:
        assert calls, "the test made no call"
        for st in calls:
            assert st["n_retried"] > 0 and st["n_batches"] > 1, st
    finally:
        P.close()


def same(got, want):
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def test_metrics(recipe, small):
    flat, seg, off = recipe
    P, calls = small
    per = TM.contig_pieces(flat)
    ws_off = np.concatenate([[0], np.cumsum([len(w) for w in per])]).astype(np.int64)
    got = P.sample_metrics(SEED, 0, S, TM.seg_array([p for w in per for p in w]), ws_off)
    calls.append(P.last_stats)
    C_ = P.n_contigs
    want = np.array([[metrics_model.words_of_array(seg[off[i * C_ + c]:off[i * C_ + c + 1]], TM.seg_array(per[c])) for c in range(C_)]
                     for i in range(S)], dtype=np.int64)
    same(got, want)
    assert got[:, :, 3].sum() > 0


@pytest.mark.parametrize("direction", TD.DIRECTIONS)
def test_distances(recipe, small, direction):
    flat, seg, off = recipe
    P, calls = small
    tracks = TD.tracks_for(flat)
    annos, anno_off = TD.csr(tracks)
    got = P.sample_distances(SEED, 0, S, annos, anno_off, 3, direction, TD.BOUND)
    calls.append(P.last_stats)
    same(got, distance_model.from_sample(seg, off, P.n_contigs, tracks, direction, TD.BOUND))
    assert got[:, :, 0].sum() > 0 and got[:, :, 1].sum() > 0


def test_signal(recipe, small):
    flat, seg, off = recipe
    P, calls = small
    tracks = TS.tracks_for(flat)
    pieces, vals, piece_off = TS.track_csr(tracks)
    got = P.sample_signal(SEED, 0, S, pieces, vals, piece_off, 3)
    calls.append(P.last_stats)
    same(got, signal_model.from_sample(seg, off, P.n_contigs, tracks))
    assert got[:, :, 0].min() > 0 and got[:, :, 1].sum() > 0


def test_local(recipe, small):
    flat, seg, off = recipe
    P, calls = small
    tracks = TL.tracks_for(flat)
    annos, anno_off = TL.csr(tracks)
    n_bins = CC.bins_for(flat, 64)
    values = local_model.from_sample(seg, off, P.n_contigs, tracks, 64, n_bins)
    obs = TL.observed_for(values)
    got, _ = P.sample_bin_enrichment(SEED, 0, S, annos, anno_off, 3, 64, n_bins, obs)
    calls.append(P.last_stats)
    same(got, local_model.words(values, obs))
    assert got[..., 1].sum() == values.sum() > 0 and got[..., 0].max() == S


def test_pairs(recipe, small):
    flat, seg, off = recipe
    P, calls = small
    tracks = TP.tracks_for(flat, 3)
    annos, anno_off = pairs_model.csr(tracks)
    values = pairs_model.from_sample(seg, off, P.n_contigs, tracks)
    obs = TP.observed_for(values)
    got = P.sample_pair_enrichment(SEED, 0, S, annos, anno_off, 3, obs)
    calls.append(P.last_stats)
    same(got, pairs_model.words(values, obs))
    assert got[:, 1].sum() == values.sum() > 0


def test_geneset(recipe, small):
    flat, seg, off = recipe
    P, calls = small
    G, T = 700, 3
    flat_genes = geneset_model.flatten(TG.genes_for(flat, G), P.n_contigs)
    terms = TG.terms_for(G, T)
    values = geneset_model.from_sample(seg, off, P.n_contigs, flat_genes, terms)
    obs = values[S // 2].copy()                     # (these lists hardly move: equal to most samples, none, and above all)
    obs[0], obs[-1] = 0, obs[-1] + 1
    pieces, piece_off, member_off, members = geneset_model.gene_csr(flat_genes)
    term_off, term_genes = geneset_model.term_csr(terms)
    got = P.sample_geneset_enrichment(SEED, 0, S, pieces, piece_off, member_off, members, G, term_off, term_genes, T, obs)
    calls.append(P.last_stats)
    same(got, geneset_model.words(values, obs))
    assert got[:, 1].sum() == values.sum() > 0


def test_profile(recipe, small):
    flat, seg, off = recipe
    P, calls = small
    anchors = TPR.anchors_for(flat)
    values = profile_model.from_sample(seg, off, P.n_contigs, anchors, TPR.BIN_SIZE, TPR.HALF_BINS, profile_model.BASES)
    obs = TPR.observed_for(values)
    pos, minus, a_off = profile_model.anchor_arrays(anchors)
    got = P.sample_profile_enrichment(SEED, 0, S, pos, minus, a_off, 3, TPR.BIN_SIZE, TPR.HALF_BINS, profile_model.BASES, obs)
    calls.append(P.last_stats)
    same(got, profile_model.words(values, obs))
    assert got[..., 1].sum() == values.sum() > 0


# ---- gat_sample_signal: the bound that grows with the slab ----------------------------------------------------------------------------
def test_signal_bound_is_checked_again_when_the_slab_grows(ctx, monkeypatch):
    """SamplerSegments without isochore keys: a base may count once per segment, so the call asks n * |q| * length < 2^63 with
    n what the contig's region of the slab holds.  A value that passes before the first batch and no longer once the regions
    have doubled: the call ends in GAT_ERR_ARG behind the repeated batch, and no row is partly written or wrong"""
    L = _lib.lib()
    p = _lib._p
    flat = CC.unit_problem("segments")
    last = int(flat["n_contigs"]) - 1                           # the contig of 150 segments: its region overflows under the knob
    assert flat["seg_off"][last + 1] - flat["seg_off"][last] == 150 and not flat["merge_contigs"]
    piece_off = np.zeros(int(flat["n_contigs"]) + 1, dtype=np.int64)
    piece_off[last + 1:] = 1
    pieces = TS.seg_array([(0, 2 ** 29)])
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(SEED, 0, S)
        assert P.last_stats["n_retried"] == 0
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    P = _lib.Problem(ctx, flat)
    try:
        st = _lib.Stats()

        def call(q, begin, end, out):
            vals = np.array([q], dtype=np.int32)
            return L.gat_sample_signal(ctx._h, P._h, SEED, begin, end, p(pieces), p(vals), p(piece_off), 1, p(out), C.byref(st))

        # the threshold, with empty ranges: the slab's bound is looked at before anything is sampled
        nothing = np.full((1, 1, 4), -1, dtype=np.int64)
        lo, hi = 1, signal_model.Q_MAX                          # lo is taken, hi refused
        assert call(lo, 0, 0, nothing) == 0 and call(hi, 0, 0, nothing) == ERR_ARG
        assert b"signal track 0:" in L.gat_last_error(ctx._h) and b"not normalized" in L.gat_last_error(ctx._h)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if call(mid, 0, 0, nothing) == 0:
                lo = mid
            else:
                hi = mid
        n_region = -(-2 ** 63 // (hi * 2 ** 29))                # what the region holds: the least n with n * hi * 2^29 >= 2^63
        assert n_region * hi * 2 ** 29 >= 2 ** 63 > n_region * lo * 2 ** 29 and n_region < 150
        assert nothing.min() == nothing.max() == -1
        q = hi * 3 // 4
        out = np.full((S, 1, 4), -1, dtype=np.int64)
        assert call(q, 0, 0, out) == 0                          # (taken as the slab is ...)
        assert call(q, 0, S, out) == ERR_ARG                    # ... and refused once it has grown
        msg = L.gat_last_error(ctx._h)
        assert b"signal track 0:" in msg and b"2^63" in msg and b"not normalized" in msg
        stats = st.asdict()
        assert stats["n_retried"] > 0
        want = signal_model.from_sample(seg, off, int(flat["n_contigs"]), [[([], [])] * last + [([(0, 2 ** 29)], [q])]])
        for i in range(S):
            assert out[i].min() == out[i].max() == -1 or out[i].tolist() == want[i].tolist(), (i, out[i].tolist(), want[i].tolist())
    finally:
        P.close()
