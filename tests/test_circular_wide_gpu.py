"""GPU: every gat_sample_* entry point on a circular problem whose sampled lists cross 2^31 and reach 2^32 - 1.

A circular problem without tracks and isochore keys takes such coordinates (sampler_takes_wide_coordinates), and that is the
problem every tool script builds.  The caller-list entry points have seen them; here they come out of the sampler, and the
host builds its windows, bins and bounds from the problem.  The contract: the words are the ones the consumer's Python model
gives on tests/circular_model.py's lists -- not on Problem.sample, which is compared with the model once -- or the call is
refused with GAT_ERR_ARG and a message that names the coordinate range.  Tracks, signal pieces, genes and anchors lie on both
sides of 2^31.  Every comparison is exact."""
import numpy as np
import pytest

import circular_cases as CIRC
import coverage_model
import distance_model
import geneset_model
import local_model
import metrics_model
import pairs_model
import profile_model
import signal_model
from gat_amd import _lib

pytestmark = pytest.mark.gpu

SEED, S = CIRC.SEED, CIRC.SAMPLES
TWO_31, TOP = CIRC.TWO_31, CIRC.TOP


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide(ctx):
    """the problem, open for the module, and the MODEL's lists of (SEED, 0, S) in Problem.sample's layout"""
    flat = CIRC.units_flat(CIRC.wide_units())
    seg, off = CIRC.model_sample(flat, SEED, 0, S)
    P = _lib.Problem(ctx, flat)
    yield P, flat, seg, off
    P.close()


def pieces_in(ws, step_div=9):
    """short pieces along every workspace piece, some of them touching: what a track looks like inside the workspace"""
    out = []
    for a, b in ws:
        step = max(3, (b - a) // step_div)
        x, k = a, 0
        while x < b:
            ln = max(1, step // 3)
            out.append((x, min(b, x + ln)))
            x += ln if k % 3 == 0 else step
            k += 1
    return [p for i, p in enumerate(out) if i == 0 or p[0] >= out[i - 1][1]]


def wide_tracks():
    """tracks[t][c]: by hand around 2^31 and at the top; short pieces along the workspace; the workspace itself, empty on the
    last contig"""
    units = CIRC.wide_units()
    hand = [[(TWO_31 - 4500, TWO_31 - 4400), (TWO_31 - 8, TWO_31 + 8), (TWO_31 + 3900, TWO_31 + 4000), (TOP - 30, TOP)],
            [(0, 50), (TWO_31 - 1, TWO_31), (TWO_31, TWO_31 + 1), (TOP - 700, TOP - 100), (TOP - 1, TOP)],
            [(TWO_31 - 2500, TWO_31 - 100), (TWO_31, TWO_31 + 1), (TWO_31 + 100, TWO_31 + 2990)]]
    fine = [pieces_in(ws) for _, ws in units]
    whole = [list(ws) for _, ws in units[:-1]] + [[]]
    return [hand, fine, whole]


def csr(entities):
    return pairs_model.csr(entities)


def test_the_tracks_lie_on_both_sides():
    for track in wide_tracks()[:2]:
        for per in track:
            assert per[0][1] <= TWO_31 <= per[-1][0] and all(x[0] < x[1] <= y[0] for x, y in zip(per, per[1:]))
    assert max(p[1] for t in wide_tracks() for per in t for p in per) == TOP


def test_sample_is_the_models(wide):
    P, flat, seg, off = wide
    got, got_off = P.sample(SEED, 0, S)
    assert got_off.tolist() == off.tolist() and got.tolist() == seg.tolist()
    assert (seg["start"] < TWO_31).any() and (seg["end"] > TWO_31).any() and seg["end"].max() == TOP


# ---- coverage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bin_size, n_bins", [(1 << 20, [4096, 4096, 2051]), (1 << 20, [2048, 2049, 2047]), (1, [5, 0, 5])],
                         ids=["2^20", "2^20-cut-at-2^31", "1-all-outside"])
def test_coverage(wide, bin_size, n_bins):
    """bins of 2^20 bases up to 2^32 (bins 2047 and 2048 meet at 2^31); the same cut at 2^31, the rest `outside`; bins of one
    base, too few of them: everything is `outside`"""
    P, flat, seg, off = wide
    n_bins = np.array(n_bins, dtype=np.int64)
    want = coverage_model.from_sample(seg, off, P.n_contigs, bin_size, n_bins)
    got = P.sample_coverage(SEED, 0, S, bin_size, n_bins)
    for g, w, name in zip(got[:4], want, ("bases", "starts", "ends", "outside")):
        assert g.tolist() == w.tolist(), name
    total = coverage_model.total_length(seg)
    assert int(got[0].sum()) + int(got[3].sum()) == total
    if bin_size == 1:
        assert int(got[3].sum()) > total - 5 * S and got[3][1] == coverage_model.total_length(
            np.concatenate([seg[off[i * 3 + 1]:off[i * 3 + 2]] for i in range(S)]))
    elif n_bins[0] == 4096:
        assert got[3].sum() == 0 and got[0][2047] > 0 and got[0][2048] > 0 and got[0][4095] > 0
        a, b = P.sample_coverage(SEED, 0, 5, bin_size, n_bins), P.sample_coverage(SEED, 5, S, bin_size, n_bins)
        assert all((x + y).tolist() == g.tolist() for x, y, g in zip(a[:4], b[:4], got[:4]))
    else:
        assert got[3].min() > 0


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def test_metrics(wide):
    """against the units' own workspaces, and against the hand-made track as a workspace the lists partly miss"""
    P, flat, seg, off = wide
    C_ = P.n_contigs
    for per in ([list(ws) for _, ws in CIRC.wide_units()], wide_tracks()[0]):
        ws, ws_off = csr([per])
        got = P.sample_metrics(SEED, 0, S, ws, ws_off)
        assert got.shape == (S, C_, len(metrics_model.WORDS))
        for i in range(S):
            for c in range(C_):
                a = seg[off[i * C_ + c]:off[i * C_ + c + 1]]
                want = metrics_model.words(list(zip(a["start"].tolist(), a["end"].tolist())), per[c])
                assert got[i, c].tolist() == want, (i, c, got[i, c].tolist(), want)
        assert got[:, :, 3].sum() > 0
    assert (got[:, :, 3] < got[:, :, 1]).any() and got[:, :, 5].sum() > 0                # (the track: bases outside it)


# ---- distances -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [0, 2 ** 32])
@pytest.mark.parametrize("direction", [distance_model.SEGMENT_TO_ANNOTATION, distance_model.ANNOTATION_TO_SEGMENT])
def test_distances(wide, direction, bound):
    """a fourth track lies at the other end of every contig: its distances need 32 bits, their sums more"""
    P, flat, seg, off = wide
    tracks = wide_tracks() + [[[(5, 9)], [(TWO_31 - 1, TWO_31)], [(TOP - 1, TOP)]]]
    annos, anno_off = csr(tracks)
    want = distance_model.from_sample(seg, off, P.n_contigs, tracks, direction, bound)
    got = P.sample_distances(SEED, 0, S, annos, anno_off, 4, direction, bound)
    assert got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert got[:, :, 0].min() > 0 and got[:, 3, 1].min() > 2 ** 31 and got[:, 3, 1].max() > 2 ** 32
    if bound:                                                                            # (whatever has a neighbour is near)
        assert (got[:, :, 2] == got[:, :, 0]).all()
    else:
        assert (got[:, :, 2] < got[:, :, 0]).any() and got[:, :, 2].sum() > 0


# ---- signal ----------------------------------------------------------------------------------------------------------------------
def test_signal(wide):
    P, flat, seg, off = wide
    r = np.random.RandomState(3)
    tracks = [[(per, [int(v) or 1 for v in r.randint(-5, 6, size=len(per))]) for per in t] for t in wide_tracks()]
    tracks[0][0][1][1] = signal_model.Q_MAX                      # the piece across 2^31 carries the largest value
    flat_pieces, piece_off = csr([[g[0] for g in t] for t in tracks])
    values = np.array([v for t in tracks for g in t for v in g[1]], dtype=np.int32)
    want = signal_model.from_sample(seg, off, P.n_contigs, tracks)
    got = P.sample_signal(SEED, 0, S, flat_pieces, values, piece_off, 3)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert got[:, :, 1].min() > 0 and np.abs(got[:, 0, 3]).max() >= signal_model.Q_MAX and got[:, :, 3].min() < 0


# ---- local -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bin_size, samples", [(1 << 20, S), (1 << 31, 3)], ids=["2^20", "2^31"])
def test_local(wide, bin_size, samples):
    """bins of 2^20 bases, and of 2^31 (two a contig; three samples: bin_size^2 * samples has to fit 64 bits)"""
    P, flat, seg, off = wide
    C_ = P.n_contigs
    tracks = wide_tracks()
    annos, anno_off = csr(tracks)
    n_bins = np.full(C_, (2 ** 32 + bin_size - 1) // bin_size, dtype=np.int64)
    values = local_model.from_sample(seg[:off[samples * C_]], off[:samples * C_ + 1], C_, tracks, bin_size, n_bins)
    obs = values[1].copy()
    obs[:, ::3] += 1
    want = local_model.words(values, obs)
    got, bin_off = P.sample_bin_enrichment(SEED, 0, samples, annos, anno_off, 3, bin_size, n_bins, obs)
    assert got.shape == want.shape and bin_off[-1] == n_bins.sum()
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    per = int(n_bins[0])
    lower, upper = got[:, :per // 2, 1].sum(), got[:, per // 2:per, 1].sum()
    assert lower > 0 and upper > 0 and got[..., 1].sum() == values.sum()                 # (both halves of contig 0)


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
def test_pairs(wide):
    P, flat, seg, off = wide
    tracks = wide_tracks()
    annos, anno_off = csr(tracks)
    values = pairs_model.from_sample(seg, off, P.n_contigs, tracks)
    obs = np.sort(values, axis=0)[S // 2].copy()
    obs[::3] = 0
    want = pairs_model.words(values, obs)
    got = P.sample_pair_enrichment(SEED, 0, S, annos, anno_off, 3, obs)
    bad = np.argwhere((got != want).any(axis=1))
    assert len(bad) == 0, (bad[0].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    assert (got[:, 0] > 0).all() and values.min(axis=0).max() > 0 and len({tuple(v) for v in values.tolist()}) > 1


# ---- gene sets -------------------------------------------------------------------------------------------------------------------
def wide_genes():
    """a gene per short piece along the workspaces, one gene across 2^31 on every contig, one at the top, one nowhere near"""
    fine = wide_tracks()[1]
    genes = [[[p] if c == cc else [] for c in range(3)] for cc in range(3) for p in fine[cc]]
    genes.append([[(TWO_31 - 50, TWO_31 + 50)]] * 3)
    genes.append([[(TOP - 5, TOP)], [(TOP - 1, TOP)], []])
    genes.append([[(5, 9)], [], [(7, 8)]])
    return genes


def test_geneset(wide):
    P, flat, seg, off = wide
    genes = wide_genes()
    G = len(genes)
    flat_genes = geneset_model.flatten(genes, P.n_contigs)
    r = np.random.RandomState(5)
    terms = [list(range(G)), list(range(0, G, 2)), [G - 3], [G - 2], [G - 1], r.choice(G, 10, replace=False).tolist()]
    values = geneset_model.from_sample(seg, off, P.n_contigs, flat_genes, terms)
    obs = np.sort(values, axis=0)[S // 2].copy()
    obs[1] = 0
    want = geneset_model.words(values, obs)
    pieces, piece_off, member_off, members = geneset_model.gene_csr(flat_genes)
    term_off, term_genes = geneset_model.term_csr(terms)
    got = P.sample_geneset_enrichment(SEED, 0, S, pieces, piece_off, member_off, members, G, term_off, term_genes, len(terms), obs)
    bad = np.argwhere((got != want).any(axis=1))
    assert len(bad) == 0, (bad[0].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    assert values[:, 2].max() == 1 and values[:, 3].max() == 1 and values[:, 4].max() == 0 and 0 < values[:, 0].min() < G


# ---- profile ---------------------------------------------------------------------------------------------------------------------
def wide_anchors():
    """anchors[t][c]: at 2^31 +- a few bases on both strands and at 2^32 - 1; inside the workspace pieces away from both"""
    return [[[(TWO_31 - 3, +1), (TWO_31 + 2, -1), (TOP, +1), (TOP, -1)], [(TWO_31, +1), (TWO_31, -1), (TOP, -1)],
             [(TWO_31 - 2, -1), (TWO_31, +1), (TWO_31 + 5, +1)]],
            [[(TWO_31 - 3500, +1), (TWO_31 + 3200, -1)], [(400, -1), (TOP - 600, +1)], [(TWO_31 - 2400, +1), (TWO_31 + 2700, -1)]],
            [[(TOP, +1)], [], []]]


@pytest.mark.parametrize("mode", [profile_model.BASES, profile_model.MIDPOINTS], ids=["bases", "midpoints"])
@pytest.mark.parametrize("bin_size, half_bins", [(25, 10), (1 << 22, 512)], ids=["w25", "w2^22-B1024"])
def test_profile(wide, mode, bin_size, half_bins):
    """windows of 250 bases either side of the anchors, and windows of 2^31 bases in 1 024 bins of 2^22"""
    P, flat, seg, off = wide
    anchors = wide_anchors()
    samples = S if bin_size == 25 else 3                 # ((K_t * bin_size)^2 * samples has to fit 64 bits)
    C_ = P.n_contigs
    values = profile_model.from_sample(seg[:off[samples * C_]], off[:samples * C_ + 1], C_, anchors, bin_size, half_bins, mode)
    obs = values[1].copy()
    obs[:, ::3] += 1
    want = profile_model.words(values, obs)
    pos, minus, a_off = profile_model.anchor_arrays(anchors)
    got = P.sample_profile_enrichment(SEED, 0, samples, pos, minus, a_off, 3, bin_size, half_bins, mode, obs)
    assert got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert (got[..., 0] > 0).any(axis=1).all()                                           # every track has a bin a sample reaches
