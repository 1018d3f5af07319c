"""GPU: k_geneset_hits and k_geneset_terms.  gat_list_geneset_hits against the model (tests/geneset_model.py) on hand-made
geometry at every bitmap-word and term-tile edge and three staging limits, gat_sample_geneset_enrichment against the model
applied to Problem.sample of the SAME problem, seed and sample range, a term of one gene per annotation interval against the
count stage's annotation-overlap, and scripts/gat-geneset.py against the table built here from Problem.sample and the model.
Every comparison is exact: integers, or the text of a table."""
import io
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import geneset_model as M
from gat_amd import _lib
from test_pairs_gpu import PROBLEMS, SAMPLES, SEED, same_words, set_options

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
GENES = (1, 31, 32, 33, 65, 2049)       # one bit; a word less one, full, plus one; three words; 65 words: past a thread per word
TERMS = (1, 63, 64, 65, 130)
PIECES = ("default", "4", "0")          # GAT_GENESET_LDS_PIECES: a group of 5 pieces and more ends in global memory at 4; 0: all of it
RUNS = ("default", "1", "5")            # GAT_GENESET_SAMPLES_PER_BLOCK
TOP = 2 ** 32 - 1
WORDS = 5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- 1. gat_list_geneset_hits -----------------------------------------------------------------------------------------------------------
def hand_genes():
    """2 049 genes over 3 groups; group 1 holds no gene"""
    r = random.Random(17)
    genes = [
        [[(100, 200)], [], [(50, 60)]],            # 0: on two contigs
        [[(300, 320)], [], []],                    # 1, 2: identical intervals
        [[(300, 320)], [], []],
        [[(400, 500)], [], []],                    # 3: cut into 5 pieces by 4 and 5
        [[(420, 430)], [], []],
        [[(460, 470)], [], []],
        [[(600, 610)], [], []],                    # 6, 7: adjacent pieces
        [[(610, 620)], [], []],
        [[], [], [(TOP - 10, TOP)]],               # 8: a piece that ends at 2^32 - 1
        [[(700, 710), (705, 720)], [], []],        # 9: given as two overlapping intervals
    ]
    genes += [[[(1000 + i, 1200 - i)], [], []] for i in range(40)]                       # 10 .. 49: a nest 40 deep
    genes += M.random_genes(r, 2049 - len(genes), [60000, 0, 5000], max_len=300)         # (those of group 0 may reach into the hand-made ones)
    return genes


def hand_lists():
    r = random.Random(23)
    unsorted = [(s, s + r.choice([1, 2, 9, 600])) for s in (r.randrange(0, 61000) for _ in range(64))]
    more = [(s, s + r.choice([1, 3, 30])) for s in (r.randrange(0, 1300) for _ in range(60))]
    return [
        [[(50, 100), (200, 250)], [(0, 100)], [(40, 50), (60, 70)]],                     # 0: bookended on both sides of gene 0 on both contigs
        [[(199, 205)], [(0, TOP)], []],                                                  # 1: one shared base with gene 0
        [[(0, TOP)], [], [(0, TOP)]],                                                    # 2: over every piece
        [[(70000, 70010)], [], [(6000, 6001)]],                                          # 3: beyond all pieces of group 0, between those of group 2
        [[], [], []],                                                                    # 4: an empty list
        [[(1100, 1101)], [], []],                                                        # 5: one segment, into the nest: one piece, 40 members
        [unsorted, [], []],                                                              # 6: 64, unsorted and overlapping
        [more + [(105, 110), (150, 160), (100, 101), (18, 12), (15, 15)], [(0, 400)], [(s, s + 25) for s in range(0, 299, 13)]],   # 7: 65 and more
    ]


def hand_terms(G, T):
    """T terms over genes 0 .. G-1: all genes, none, one, 64, 65 (as far as G goes), gene 0 in terms 5 .. 44, random ones"""
    r = random.Random(1000 * G + T)
    terms = [list(range(G)), [], [0], list(range(min(G, 64))), list(range(G - min(G, 65), G))]
    while len(terms) < T:
        t = r.sample(range(G), min(G, r.choice([1, 2, 10, 10, 10, 70, 300])))
        terms.append(sorted(set(t + ([0] if len(terms) < 45 else []))))
    return terms[:T]


@pytest.fixture(scope="module")
def geometry():
    """the genes and the lists, and per G the model's pieces -- flattened once"""
    genes, lists = hand_genes(), hand_lists()
    return dict(genes=genes, lists=lists, flat=dict((G, M.flatten(genes[:G], 3)) for G in GENES))


def test_hand_geometry_is_what_it_says(geometry):
    genes, lists, flat = geometry["genes"], geometry["lists"], geometry["flat"][2049]
    assert len(genes) == 2049 and all(len(per) == 3 and not per[1] for per in genes) and not flat[1]
    assert genes[1] == genes[2] and genes[0][0] and genes[0][2]
    assert [sum(len(x) for x in l) for l in lists] == [5, 2, 2, 2, 0, 1, 64, 60 + 5 + 1 + 23]
    assert len(lists[7][0]) == 65 and not M.is_normalized(lists[6][0])
    hand = M.flatten(genes[:50], 3)
    assert all(M.is_normalized([(a, b) for a, b, _ in per]) for per in flat)
    assert sum(1 for _, _, who in hand[0] if 3 in who) == 5                                  # gene 3 in 5 pieces
    assert max(len(who) for _, _, who in hand[0]) == 40 > 4                                  # the nest
    assert any(p[1] == q[0] for p, q in zip(flat[0][:-1], flat[0][1:]))                      # adjacent pieces
    assert flat[2][-1][1] == TOP and (700, 720, [9]) in hand[0]
    H = [M.hit_set(l, hand) for l in lists]
    assert H[0] == set() and H[1] == {0} and H[2] == set(range(50)) and H[3] == set() and H[4] == set() and H[5] == set(range(10, 50))
    assert all(M.hit_set(l, flat) == M.brute_hit_set(l, genes) for l in (lists[1], lists[6]))
    # gene 0 is hit by three segments of list 7 and on two contigs, and is counted once; some term is hit in part
    assert sum(1 for s, e in lists[7][0] if e > s and s < 200 and e > 100) >= 3 and lists[7][2][3] == (39, 64)
    terms = hand_terms(2049, 130)
    c = M.all_counts(lists, flat, terms)
    assert c[7, 2] == 1 and c[1, 2] == 1 and 0 < c[6, 0] < 2049 and c[2].tolist() == [len(set(t)) for t in terms]
    assert [len(t) for t in terms[:5]] == [2049, 0, 1, 64, 65] and sum(1 for t in terms if 0 in t) >= 40 + 3
    assert [len(t) for t in hand_terms(65, 5)] == [65, 0, 1, 64, 65]


@pytest.mark.parametrize("T", TERMS)
@pytest.mark.parametrize("G", GENES)
def test_list_geneset_hits(ctx, monkeypatch, geometry, G, T):
    """the model's counts, whatever the staging limit and the run"""
    lists, flat = geometry["lists"], geometry["flat"][G]
    terms = hand_terms(G, T)
    want = M.all_counts(lists, flat, terms)
    assert want.sum() > 0 and want[2, 0] == G
    a, a_off = M.csr(lists)
    pieces, piece_off, member_off, members = M.gene_csr(flat)
    term_off, term_genes = M.term_csr(terms)
    for pieces_knob in PIECES:
        for run in ("default", "1"):
            set_options(ctx, monkeypatch, GAT_GENESET_LDS_PIECES=pieces_knob, GAT_GENESET_SAMPLES_PER_BLOCK=run)
            got = ctx.list_geneset_hits(a, a_off, len(lists), pieces, piece_off, member_off, members, G, term_off, term_genes, T, 3)
            assert got.dtype == np.int64 and got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (G, T, pieces_knob, run, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))
    # the term tile changes nothing either
    set_options(ctx, monkeypatch, GAT_GENESET_LDS_PIECES="default", GAT_GENESET_SAMPLES_PER_BLOCK="default", GAT_GENESET_TERM_TILE="7")
    got = ctx.list_geneset_hits(a, a_off, len(lists), pieces, piece_off, member_off, members, G, term_off, term_genes, T, 3)
    assert np.array_equal(got, want)
    # nor does a scratch budget that holds the bitmaps of one list (2 049 genes: 260 bytes) or of a few: the lists go in chunks
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "2000" if G > 65 else "100")
    got = ctx.list_geneset_hits(a, a_off, len(lists), pieces, piece_off, member_off, members, G, term_off, term_genes, T, 3)
    assert np.array_equal(got, want)


def small_case():
    flat = M.flatten([[[(0, 4), (20, 32)]], [[(2, 8)]]], 1)                      # pieces (0,2,[0]) (2,4,[0,1]) (4,8,[1]) (20,32,[0])
    return M.csr([[[(1, 2), (30, 40), (8, 9)]]]), M.gene_csr(flat), M.term_csr([[0], [1], [0, 1]])


def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    (segs, off), (pieces, piece_off, member_off, members), (term_off, term_genes) = small_case()
    out = np.full((1, 3), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, pc=pieces, po=piece_off, mo=member_off, m=members, ng=2, to=term_off, tg=term_genes, t=3,
             g=1, o=out):
        return L.gat_list_geneset_hits(c, p(lists), p(lo), n, p(pc), p(po), p(mo), p(m), ng, p(to), p(tg), t, g, p(o))

    assert call() == 0 and out.tolist() == [[1, 0, 1]]
    keep = out.copy()
    i64 = lambda *x: np.array(x, dtype=np.int64)                                         # noqa: E731
    i32 = lambda *x: np.array(x, dtype=np.int32)                                         # noqa: E731
    for bad in (dict(c=None), dict(lo=None), dict(po=None), dict(mo=None), dict(to=None), dict(o=None), dict(lists=None), dict(pc=None),
                dict(m=None), dict(tg=None), dict(n=-1), dict(t=-1), dict(g=-1), dict(ng=-1), dict(lo=i64(2, 0)), dict(po=i64(4, 0)),
                dict(mo=i64(0, 1, 3, 2, 5)), dict(to=i64(0, 1, 0, 4))):
        assert call(**bad) == -6, bad
        assert np.array_equal(out, keep)
    err = lambda: L.gat_last_error(ctx._h)                                               # noqa: E731
    assert call(ng=262145) == -6 and b"n_genes 262145 outside [0, 262144]" in err()
    assert call(mo=i64(0, 1, 3, 2, 5)) == -6 and b"member_off decreases at piece 2" in err()
    assert call(mo=i64(0, 1, 3, 3, 5)) == -6 and b"piece 2 has no member" in err()
    assert call(to=i64(0, 1, 0, 4)) == -6 and b"term_off decreases at term 1" in err()
    assert call(m=i32(0, 0, 2, 1, 0)) == -6 and b"the members of piece 1 are not strictly ascending gene ids in [0, 2)" in err()
    assert call(m=i32(0, 1, 0, 1, 0)) == -6 and b"the members of piece 1" in err()
    assert call(m=i32(0, 0, 1, 1, -1)) == -6 and b"the members of piece 3" in err()
    assert call(tg=i32(0, 1, 1, 0)) == -6 and b"the genes of term 2 are not strictly ascending" in err()
    assert call(tg=i32(0, 2, 0, 1)) == -6 and b"the genes of term 1" in err()
    # the pieces must be normalized, and the message names the group and the piece; a segment list need not be
    for bad in ([(0, 2), (1, 4), (4, 8), (20, 32)], [(2, 4), (0, 2), (4, 8), (20, 32)], [(0, 2), (2, 4), (6, 6), (20, 32)]):
        assert call(pc=M.csr([[bad]])[0]) == -6 and b"gene pieces 0, group 0 is not normalized at interval" in err()
    assert call(lists=M.csr([[[(0, 4), (3, 8), (6, 6)]]])[0]) == 0 and out.tolist() == [[1, 1, 2]]
    out[:] = keep
    two = M.gene_csr([[(0, 4, [0])], [(5, 9, [1]), (8, 12, [0])]])
    l2, lo2 = M.csr([[[(0, 4)], [(2, 30)]]])
    assert call(lists=l2, lo=lo2, pc=two[0], po=two[1], mo=two[2], m=two[3], g=2) == -6
    assert b"gene pieces 0, group 1 is not normalized at interval 1" in err()
    assert np.array_equal(out, keep)
    assert call(t=0, to=i64(0)) == 0 and call(n=0) == 0 and np.array_equal(out, keep)     # nothing to write
    out[:] = -1
    assert call() == 0 and np.array_equal(out, keep)                                       # the context is still good


# ---- 2. gat_sample_geneset_enrichment ---------------------------------------------------------------------------------------------------
SAMPLE_GENES = (40, 700)
SAMPLE_TERMS = (3, 66)


def genes_for(flat, G, seed=9):
    """G genes over the contigs of a problem: one to three intervals each, of up to a fortieth of the contig"""
    r = random.Random(seed + G)
    spans = [max(50, int(x)) for x in CC.extents(flat)]
    return M.random_genes(r, G, spans, max_len=max(2, min(spans) // 40))


def terms_for(G, T, seed=3):
    r = random.Random(seed + 7 * G + T)
    terms = [list(range(G)), r.sample(range(G), G // 2), r.sample(range(G), G // 3)]
    while len(terms) < T:
        terms.append(r.sample(range(G), min(G, r.choice([0, 1, 3, 10, 10, 70]))))
    return terms[:T]


def observed_for(values):
    """an obs per term that meets every branch: the median of the term's sample values, 0 for every third term, max + 1 for
    every fifth, and the maximum for the last term whose values differ (some samples below it, some equal)"""
    obs = np.sort(values, axis=0)[len(values) // 2].copy()
    obs[::3] = 0
    obs[1::5] = values.max(axis=0)[1::5] + 1
    varying = np.flatnonzero(values.min(axis=0) < values.max(axis=0))
    assert len(varying) > 0
    obs[varying[-1]] = values[:, varying[-1]].max()
    return obs


@pytest.fixture(scope="module")
def sampled(ctx):
    """per problem: the flat problem, Problem.sample of (SEED, 0, SAMPLES) -- drawn once --, and per (G, T) the genes' pieces, the
    terms and the model's counts [samples][T] of those lists"""
    cache = {}

    def get(name, G=None, T=None):
        if name not in cache:
            flat = CC.SIX[name]()
            P = _lib.Problem(ctx, flat)
            try:
                seg, off = P.sample(SEED, 0, SAMPLES)
                n_contigs = P.n_contigs
            finally:
                P.close()
            cache[name] = dict(flat=flat, seg=seg, off=off, n_contigs=n_contigs, pieces={}, values={})
        e = cache[name]
        if G is not None and (G, T) not in e["values"]:
            if G not in e["pieces"]:
                e["pieces"][G] = M.flatten(genes_for(e["flat"], G), e["n_contigs"])
            terms = terms_for(G, T)
            e["values"][G, T] = (terms, M.from_sample(e["seg"], e["off"], e["n_contigs"], e["pieces"][G], terms))
        return e
    return get


def sample_call(P, e, G, T, obs, begin=0, end=SAMPLES):
    terms = e["values"][G, T][0]
    pieces, piece_off, member_off, members = M.gene_csr(e["pieces"][G])
    term_off, term_genes = M.term_csr(terms)
    return P.sample_geneset_enrichment(SEED, begin, end, pieces, piece_off, member_off, members, G, term_off, term_genes, T, obs)


@pytest.mark.parametrize("T", SAMPLE_TERMS)
@pytest.mark.parametrize("G", SAMPLE_GENES)
@pytest.mark.parametrize("name", PROBLEMS)
def test_samplers(ctx, sampled, monkeypatch, name, G, T):
    e = sampled(name, G, T)
    terms, values = e["values"][G, T]
    obs = observed_for(values)
    want = M.words(values, obs)
    P = _lib.Problem(ctx, e["flat"])
    try:
        for run in RUNS:                                # one batch: runs of 1, of 5 (the last one short), and the launch's own
            set_options(ctx, monkeypatch, GAT_GENESET_SAMPLES_PER_BLOCK=run)
            same_words(sample_call(P, e, G, T, obs), want, (name, G, T, run))
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "20000")                 # a scratch budget of a few samples: several batches
    P = _lib.Problem(ctx, e["flat"])
    try:
        got = sample_call(P, e, G, T, obs)
        assert P.last_stats["n_batches"] >= 2, P.last_stats["n_batches"]
        same_words(got, want, (name, G, T, "batches"))
        # not vacuous: every branch of the comparison with obs
        n_less, n_eq = got[:, 3], got[:, 4]
        assert ((n_less > 0) & (n_less < SAMPLES)).any() and ((n_eq > 0) & (n_eq < SAMPLES)).any()
        assert (n_less == SAMPLES).any() and (n_less + n_eq <= SAMPLES).all() and got[:, 1].sum() == values.sum() > 0
        assert (values[:, 0] < G).any() and (got[:, 0] < SAMPLES).any() == bool((values == 0).any())
    finally:
        P.close()
    if name == "segments-genome":              # SamplerSegments without isochore keys: lists neither sorted nor disjoint, and taken
        assert not all(M.is_normalized(e["seg"][e["off"][l]:e["off"][l + 1]]) for l in range(len(e["off"]) - 1))


# ---- 3. additivity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SAMPLE_TERMS)
def test_additive_over_the_range(ctx, sampled, monkeypatch, T):
    """[0, k) plus [k, S) is [0, S), for k in the middle of a batch"""
    G = 700
    e = sampled("annotator-genome-isochores", G, T)
    terms, values = e["values"][G, T]
    obs = observed_for(values)
    P = _lib.Problem(ctx, e["flat"])
    try:
        for shift in range(16):                         # a scratch budget that takes the range in 2 to 16 batches of 3 samples and more
            monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", str(20000 << shift))
            whole = sample_call(P, e, G, T, obs)
            n_batches = P.last_stats["n_batches"]
            if n_batches <= SAMPLES // 3:
                break
        sizes = [b for b in range(1, SAMPLES + 1) if -(-SAMPLES // b) == n_batches]      # what a batch may hold, given their number
        assert n_batches >= 2 and sizes and min(sizes) >= 3, (n_batches, sizes)
        k = [k for k in range(1, SAMPLES) if all(k % b for b in sizes)][len(sizes) // 2]
        first = sample_call(P, e, G, T, obs, 0, k)
        rest = sample_call(P, e, G, T, obs, k, SAMPLES)
    finally:
        P.close()
    same_words(whole, M.words(values, obs), "whole")
    same_words(first, M.words(values[:k], obs), "[0, %d)" % k)
    assert np.array_equal(first + rest, whole)


def test_a_batch_in_chunks_of_bitmaps(ctx, sampled, monkeypatch):
    """200 000 genes (all but 40 without an interval) are 25 000 bytes of bitmap a sample; a quarter of a scratch budget of 400 000
    bytes holds four, and a batch of more samples than that goes through both kernels in chunks"""
    G, T, n_genes = 40, 66, 200000
    e = sampled("annotator-units", G, T)
    terms, values = e["values"][G, T]
    obs = observed_for(values)
    pieces, piece_off, member_off, members = M.gene_csr(e["pieces"][G])
    term_off, term_genes = M.term_csr(terms)
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "400000")
    P = _lib.Problem(ctx, e["flat"])
    try:
        got = P.sample_geneset_enrichment(SEED, 0, SAMPLES, pieces, piece_off, member_off, members, n_genes, term_off, term_genes, T, obs)
        assert 400000 // 4 // (n_genes // 8) == 4 < -(-SAMPLES // P.last_stats["n_batches"])       # (a batch holds more than a chunk)
    finally:
        P.close()
    same_words(got, M.words(values, obs), "chunks")


# ---- 4. against the count stage ---------------------------------------------------------------------------------------------------------
def test_term_of_a_tracks_intervals_is_annotation_overlap(ctx):
    """every interval of a problem's own (normalized) annotation track a gene, the track's genes a term: c is the intervals of
    the track hit by a segment, which on normalized lists is CounterAnnotationOverlap -- checked against the oracle in
    tests/test_geneset_host.py -- and the count stage gives that per sample"""
    from gat_amd import problem, synthetic
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], None)
    annos, anno_off, T, C_, S = flat["annos"], flat["anno_off"], int(flat["n_tracks"]), int(flat["n_contigs"]), 40
    assert T >= 3 and len(anno_off) == T * C_ + 1
    genes, terms = [], []
    for t in range(T):
        first = len(genes)
        for c in range(C_):
            a = annos[anno_off[t * C_ + c]:anno_off[t * C_ + c + 1]]
            assert M.is_normalized(a)
            genes.extend([[(int(s), int(e))] if g == c else [] for g in range(C_)] for s, e in zip(a["start"], a["end"]))
        terms.append(list(range(first, len(genes))))
    assert all(len(t) > 0 for t in terms)
    pieces, piece_off, member_off, members = M.gene_csr(M.flatten(genes, C_))
    term_off, term_genes = M.term_csr(terms)
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(SEED, 0, S)
        assert all(M.is_normalized(seg[off[l]:off[l + 1]]) for l in range(len(off) - 1))
        counts = P.sample_and_count(["annotation-overlap"], SEED, 0, S)[0]
        assert counts.shape == (T, S) and counts.sum() > 0
        got = P.sample_geneset_enrichment(SEED, 0, S, pieces, piece_off, member_off, members, len(genes), term_off, term_genes, T,
                                          np.zeros(T, dtype=np.int64))
    finally:
        P.close()
    for t in range(T):
        assert got[t, 1] == counts[t].sum() and got[t, 0] == (counts[t] > 0).sum() and got[t, 2] == (counts[t] * counts[t]).sum()


# ---- 5. error paths ---------------------------------------------------------------------------------------------------------------------
def test_sample_arguments(ctx, sampled):
    L = _lib.lib()
    p = _lib._p
    G, T = 40, 3
    e = sampled("annotator-units", G, T)
    terms, values = e["values"][G, T]
    pieces, piece_off, member_off, members = M.gene_csr(e["pieces"][G])
    term_off, term_genes = M.term_csr(terms)
    obs = observed_for(values)
    P = _lib.Problem(ctx, e["flat"])
    try:
        out = np.full((T, WORDS), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, pc=pieces, po=piece_off, mo=member_off, m=members, ng=G, to=term_off, tg=term_genes,
                 t=T, ob=obs, o=out):
            return L.gat_sample_geneset_enrichment(c, prob, SEED, begin, end, p(pc), p(po), p(mo), p(m), ng, p(to), p(tg), t, p(ob), p(o), None)

        err = lambda: L.gat_last_error(ctx._h)                                           # noqa: E731
        assert call() == 0
        same_words(out, M.words(values[:2], obs), "two samples")
        keep = out.copy()
        down_p, down_m, down_t = piece_off.copy(), member_off.copy(), term_off.copy()
        down_p[1] = down_p[-1] + 1
        down_m[2] = down_m[1] - 1
        down_t[1] = down_t[2] + 1
        negative = obs.copy()
        negative[1] = -1
        bad_members, bad_terms = members.copy(), term_genes.copy()
        bad_members[0] = G
        bad_terms[int(term_off[1])] = -1
        for bad in (dict(c=None), dict(prob=None), dict(po=None), dict(mo=None), dict(to=None), dict(ob=None), dict(o=None), dict(pc=None),
                    dict(m=None), dict(tg=None), dict(begin=3, end=2), dict(t=-1), dict(ng=-1), dict(po=down_p), dict(mo=down_m), dict(to=down_t),
                    dict(ob=negative), dict(ng=262145), dict(m=bad_members), dict(tg=bad_terms)):
            assert call(**bad) == -6, bad
        assert b"obs[1] = -1 is negative" in (call(ob=negative), err())[1]
        assert b"outside [0, 262144]" in (call(ng=262145), err())[1]
        assert b"the members of piece 0" in (call(m=bad_members), err())[1] and b"the genes of term 1" in (call(tg=bad_terms), err())[1]
        # sumsq must fit: n_genes^2 * samples < 2^64
        assert call(end=-(-2 ** 64 // (G * G))) == -6 and b"sumsq" in err()
        # pieces that are not normalized are named: the group (the problem's contig) and the piece
        c2 = [c for c in range(P.n_contigs) if piece_off[c + 1] - piece_off[c] >= 2][-1]
        bad_pieces = pieces.copy()
        at = int(piece_off[c2])
        bad_pieces["start"][at + 1] = bad_pieces["end"][at] - 1
        assert call(pc=bad_pieces) == -6 and ("gene pieces 0, group %d is not normalized at interval 1" % c2).encode() in err()
        assert np.array_equal(out, keep)                                                   # no refused call wrote anything
        assert call(t=0, to=np.zeros(1, dtype=np.int64), ob=None, o=None) == 0             # no term: nothing to write
        assert call() == 0 and np.array_equal(out, keep)
        out[:] = -1
        assert call(begin=4, end=4) == 0 and out.min() == out.max() == 0                   # an empty range writes zeros
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], SEED, 0, 2, dev)
            assert call() == -6 and b"in flight" in err()
            P.wait()
        finally:
            ctx.free(dev)
        assert out.min() == out.max() == 0
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        pieces, piece_off, member_off, members = M.gene_csr(M.flatten([[[(1, 2)] for _ in range(P.n_contigs)]], P.n_contigs))
        term_off, term_genes = M.term_csr([[0]])
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_geneset_enrichment(1, 0, 1, pieces, piece_off, member_off, members, 1, term_off, term_genes, 1, np.zeros(1, dtype=np.int64))
    finally:
        P.close()


# ---- 6. the script ----------------------------------------------------------------------------------------------------------------------
CLI_SEED, CLI_SAMPLES = 11, 30


@pytest.mark.parametrize("extra", [["--isochores=%s" % os.path.join(CLI, "isochores.bed"), "--order=track"],
                                   ["--with-segment-tracks", "--qvalue-method=holm", "--order=pvalue"], ["--sampler=circular"]],
                         ids=["isochores", "tracks", "circular"])
def test_script(ctx, tmp_path, extra):
    """the printed table is the one built here: Problem.sample of the same inputs and seeds, the model's counts and words"""
    from gat_amd import geneset, problem
    from test_geneset_host import script, write_cli_genes
    mod = script()
    genes_file, map_file = write_cli_genes(tmp_path)
    argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--genes=%s" % genes_file, "--gene-sets=%s" % map_file,
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % CLI_SAMPLES, "--random-seed=%d" % CLI_SEED,
            "--min-term-genes=2", "--verbose=0"] + extra
    assert mod.main(["gat-geneset.py", "--stdout=%s" % (tmp_path / "got.tsv")] + argv) == 0
    opts, _ = mod.buildParser().parse_args(argv)
    segments, annotations, workspace = geneset.build_inputs(opts)
    ids, genes, dropped = geneset.gene_table(annotations)
    names, term_off, term_genes, unknown = geneset.term_table(geneset.read_gene_sets(map_file), ids)
    assert len(ids) >= 10 and len(names) >= 4 and unknown == 1 + dropped
    terms = [term_genes[term_off[t]:term_off[t + 1]].tolist() for t in range(len(names))] + [list(range(len(ids)))]
    results = []
    seed = CLI_SEED
    for track in segments.tracks:
        flat, sa, wa = geneset.flatten(segments[track], workspace, geneset.make_sampler(opts))
        contigs = list(flat["contig_names"])
        csegs = problem.from_isochores(sa)
        pieces = M.flatten([[[(int(s), int(e)) for s, e in zip(per[c]["start"], per[c]["end"])] if c in per else [] for c in contigs]
                            for per in genes], len(contigs))
        P = _lib.Problem(ctx, flat)
        try:
            seg, off = P.sample(seed, 0, CLI_SAMPLES)
        finally:
            P.close()
        seed = (seed + CLI_SAMPLES * int(flat["n_units"])) & 0xFFFFFFFF
        obs = M.all_counts([[csegs.get(c, []) for c in contigs]], pieces, terms)[0]
        words = M.words(M.from_sample(seg, off, len(contigs), pieces, terms), obs)
        results.extend(geneset.rows(track, names, term_off, len(ids), obs, words, CLI_SAMPLES, min_term_genes=2))
    geneset.set_qvalues(results, opts.qvalue_method)
    sink = io.StringIO()
    geneset.write_results(sink, results, opts.output_order)
    got = "".join(l for l in open(str(tmp_path / "got.tsv")) if not l.startswith("#"))
    assert got == sink.getvalue()
    rows = [l.split("\t") for l in got.splitlines()[1:]]
    assert len(rows) >= 2 and all(len(r) == 17 for r in rows) and all(int(r[3]) >= 2 for r in rows)
    assert any(int(r[5]) > 0 and float(r[6]) > 0 for r in rows) and any(0 < int(r[5]) < int(r[3]) for r in rows)
