"""CPU: the model of the gene-set hits (tests/geneset_model.py) against a literal double loop over (segment, gene interval), and
geneset.flatten_genes against the model's sweep and against the bases themselves."""
import random

import numpy as np
import pytest

import geneset_model as M


def random_lists(r, n_lists, spans, n_max=12):
    return [[[(s, s + r.choice([-2, 0, 1, 2, 9, 60])) for s in (r.randrange(0, max(1, span)) for _ in range(r.randint(0, n_max)))]
             for span in spans] for _ in range(n_lists)]


@pytest.mark.parametrize("seed", range(6))
def test_model_is_the_double_loop(seed):
    r = random.Random(seed)
    spans = [300, 0, 120]
    genes = M.random_genes(r, r.choice([1, 7, 40]), spans)
    flat = M.flatten(genes, len(spans))
    terms = [r.sample(range(len(genes)), r.randint(0, len(genes))) for _ in range(9)] + [range(len(genes)), []]
    lists = random_lists(r, 8, spans)
    want = np.array([[len(M.brute_hit_set(l, genes) & set(t)) for t in terms] for l in lists], dtype=np.int64)
    got = M.all_counts(lists, flat, terms)
    assert np.array_equal(got, want) and (want.sum() > 0 or len(genes) == 1)
    for l in lists:
        assert M.hit_set(l, flat) == M.brute_hit_set(l, genes)
        assert np.array_equal(M.counts(l, flat, terms), M.all_counts([l], flat, terms)[0])


def test_model_on_hand_cases():
    genes = [[[(10, 20)]], [[(10, 20)]], [[(15, 40), (12, 18)]], [[(100, 101)]]]       # two identical genes; one of two overlapping lines
    flat = M.flatten(genes, 1)
    assert flat == [[(10, 12, [0, 1]), (12, 20, [0, 1, 2]), (20, 40, [2]), (100, 101, [3])]]
    for seg, want in (([(0, 10)], set()), ([(20, 21)], {2}), ([(9, 11)], {0, 1}), ([(40, 100)], set()), ([(40, 101)], {3}),
                      ([(19, 20), (19, 20), (11, 30)], {0, 1, 2}), ([(30, 12)], set()), ([(15, 15)], set()), ([(0, 2 ** 32 - 1)], {0, 1, 2, 3})):
        assert M.hit_set([seg], flat) == want == M.brute_hit_set([seg], genes), seg
    pieces, piece_off, member_off, members = M.gene_csr(flat)
    assert piece_off.tolist() == [0, 4] and member_off.tolist() == [0, 2, 5, 6, 7] and members.tolist() == [0, 1, 0, 1, 2, 2, 3]
    assert M.term_csr([[3, 1, 1], [], [0]])[0].tolist() == [0, 2, 2, 3] and M.term_csr([[3, 1, 1], [], [0]])[1].tolist() == [1, 3, 0]
    v = np.array([[0, 2], [1, 2], [3, 0]], dtype=np.int64)
    assert M.words(v, np.array([1, 2])).tolist() == [[2, 4, 10, 1, 1], [2, 4, 8, 1, 2]]


# ---- geneset.flatten_genes ------------------------------------------------------------------------------------------------------------
def as_dicts(genes, contigs):
    return [dict((contigs[g], per[g]) for g in range(len(contigs)) if per[g]) for per in genes]


@pytest.mark.parametrize("seed", range(5))
def test_flatten_genes_base_by_base(seed):
    """on contigs of 400 bases: the pieces are normalized, their union is the union of the genes, and the members of the piece
    that holds a base are exactly the genes that cover the base"""
    from gat_amd import geneset
    r = random.Random(100 + seed)
    contigs, spans = ["chrA", "chrEmpty", "chrB"], [400, 0, 400]
    genes = M.random_genes(r, r.choice([1, 9, 60]), spans, max_len=r.choice([5, 90]))
    pieces, piece_off, member_off, members = geneset.flatten_genes(as_dicts(genes, contigs), contigs)
    assert pieces.dtype == M.SEG and members.dtype == np.int32 and piece_off.dtype == member_off.dtype == np.int64
    assert piece_off[0] == 0 and piece_off[1] == piece_off[2] and len(member_off) == piece_off[-1] + 1 and member_off[-1] == len(members)
    for g in (0, 2):
        mine = pieces[piece_off[g]:piece_off[g + 1]]
        assert M.is_normalized(mine)
        cover = [set() for _ in range(400)]
        for k, per in enumerate(genes):
            for s, e in per[g]:
                for x in range(s, e):
                    cover[x].add(k)
        seen = [set() for _ in range(400)]
        for j in range(int(piece_off[g]), int(piece_off[g + 1])):
            who = members[member_off[j]:member_off[j + 1]].tolist()
            assert who and who == sorted(set(who))
            for x in range(int(pieces["start"][j]), int(pieces["end"][j])):
                assert not seen[x]
                seen[x] = set(who)
        assert seen == cover
        # elementary: a piece ends where the set of genes changes, or where no gene goes on
        for j in range(int(piece_off[g]), int(piece_off[g + 1]) - 1):
            if pieces["end"][j] == pieces["start"][j + 1]:
                assert members[member_off[j]:member_off[j + 1]].tolist() != members[member_off[j + 1]:member_off[j + 2]].tolist()
    # and it is the model's sweep
    want = M.gene_csr(M.flatten(genes, 3))
    for a, b in zip((pieces, piece_off, member_off, members), want):
        assert np.array_equal(a, b)


def test_flatten_genes_merges_a_genes_own_lines():
    from gat_amd import geneset
    two = geneset.flatten_genes([{"c": [(10, 30), (20, 50)]}, {"c": [(40, 60)]}], ["c"])
    one = geneset.flatten_genes([{"c": [(10, 50)]}, {"c": [(40, 60)]}], ["c"])
    for a, b in zip(two, one):
        assert np.array_equal(a, b)
    assert [tuple(p) for p in two[0].tolist()] == [(10, 40), (40, 50), (50, 60)] and two[3].tolist() == [0, 0, 1, 1]
    none = geneset.flatten_genes([], ["c", "d"])
    assert len(none[0]) == 0 and none[1].tolist() == [0, 0, 0] and none[2].tolist() == [0] and len(none[3]) == 0
    # adjacent intervals of one gene are one; a contig the call does not name is left out
    adj = geneset.flatten_genes([{"c": [(5, 9), (9, 12)], "other": [(1, 2)]}], ["c"])
    assert [tuple(p) for p in adj[0].tolist()] == [(5, 12)] and adj[3].tolist() == [0]
