"""Plain model of the gene-set hits (gat_list_geneset_hits / gat_sample_geneset_enrichment).  TEST INFRASTRUCTURE ONLY.

genes[g][group] is a list of (start, end) intervals of gene g, in any order, overlapping or not.  A segment q = [s, e), e > s,
hits gene g when it shares a base with one of its intervals (on the segment's group).  H(L) is the SET of genes hit by any
segment of list L over all its groups, c(L, t) = |H(L) & M_t| for term t with gene set M_t.  Everything here is Python sets and
loops; `flatten` makes the pieces and members the library takes, by a sweep over the boundaries.
"""
import numpy as np

from local_model import pairs as as_pairs     # a list as an int64 array [n, 2]
from local_model import is_normalized, words  # noqa: F401  (the five words are gat-local's: words(values [S][T], obs [T]))

WORDS = ("n_pos", "sum", "sumsq", "n_less", "n_eq")
SEG = np.dtype([("start", "<u4"), ("end", "<u4")])


def merged(intervals):
    """a gene's own intervals as one sorted list without overlapping or adjacent ones"""
    out = []
    for s, e in sorted((int(s), int(e)) for s, e in intervals if e > s):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def flatten(genes, n_groups):
    """-> per group the list of (start, end, sorted gene ids): the elementary intervals between consecutive boundaries of the
    genes (each gene's own intervals merged first) that a gene covers"""
    out = []
    for g in range(n_groups):
        ivs = [(s, e, k) for k, per in enumerate(genes) for s, e in merged(as_pairs(per[g]).tolist())]
        bounds = sorted(set([s for s, _, _ in ivs] + [e for _, e, _ in ivs]))
        begin, finish = {}, {}
        for s, e, k in ivs:
            begin.setdefault(s, []).append(k)
            finish.setdefault(e, []).append(k)
        pieces, open_now = [], {}                    # open_now[k]: intervals of gene k that cover the bases from `a` on
        for a, b in zip(bounds[:-1], bounds[1:]):
            for k in finish.get(a, ()):
                open_now[k] -= 1
                if open_now[k] == 0:
                    del open_now[k]
            for k in begin.get(a, ()):
                open_now[k] = open_now.get(k, 0) + 1
            if open_now:
                pieces.append((a, b, sorted(open_now)))
        out.append(pieces)
    return out


def gene_csr(flat):
    """flatten's pieces -> (pieces SEG, piece_off, member_off, members int32) as the C ABI takes them"""
    rows = [p for per in flat for p in per]
    pieces = np.zeros(len(rows), dtype=SEG)
    pieces["start"], pieces["end"] = [p[0] for p in rows], [p[1] for p in rows]
    piece_off = np.concatenate([[0], np.cumsum([len(per) for per in flat])]).astype(np.int64)
    member_off = np.concatenate([[0], np.cumsum([len(p[2]) for p in rows])]).astype(np.int64)
    members = np.array([k for p in rows for k in p[2]], dtype=np.int32)
    return pieces, piece_off, member_off, members


def term_csr(terms):
    """terms[t]: iterable of gene ids -> (term_off, term_genes int32), ascending and duplicate-free per term"""
    lists = [sorted(set(int(k) for k in t)) for t in terms]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, np.array([k for x in lists for k in x], dtype=np.int32)


def csr(lists_of_lists):
    """entity-major lists[e][g] -> (SEG array, offsets) as the C ABI takes them"""
    flat = [as_pairs(a) for per in lists_of_lists for a in per]
    off = np.zeros(len(flat) + 1, dtype=np.int64)
    if flat:
        np.cumsum([len(a) for a in flat], out=off[1:])
    seg = np.zeros(int(off[-1]), dtype=SEG)
    if len(seg):
        allp = np.concatenate(flat, axis=0)
        seg["start"], seg["end"] = allp[:, 0].astype(np.uint32), allp[:, 1].astype(np.uint32)
    return seg, off


def hit_set(per_list, flat):
    """H(L): per_list[g] the segments of group g, flat = flatten(genes): found through the pieces, the way the definition puts
    it -- the members of the pieces from the first with end > s up to the first with start >= e"""
    H = set()
    for g, seg in enumerate(per_list):
        pieces = flat[g]
        if not pieces:
            continue
        ends = np.array([p[1] for p in pieces], dtype=np.int64)
        starts = np.array([p[0] for p in pieces], dtype=np.int64)
        for s, e in as_pairs(seg).tolist():
            if e <= s:
                continue
            j0 = int(np.searchsorted(ends, s, side="right"))
            j1 = int(np.searchsorted(starts, e, side="left"))
            for j in range(j0, j1):
                H.update(pieces[j][2])
    return H


def counts(per_list, flat, terms):
    """c(L, t) for every term: int64 [T]"""
    H = hit_set(per_list, flat)
    return np.array([len(H & set(int(k) for k in t)) for t in terms], dtype=np.int64)


def all_counts(lists, flat, terms):
    """lists[l][g] -> int64 [n_lists][T]"""
    out = np.zeros((len(lists), len(terms)), dtype=np.int64)
    sets = [set(int(k) for k in t) for t in terms]
    for l, per_list in enumerate(lists):
        H = hit_set(per_list, flat)
        out[l] = [len(H & m) for m in sets]
    return out


def from_sample(seg, off, n_contigs, flat, terms):
    """the counts of every sample of a Problem.sample: seg / off as returned (sample-major, n_contigs lists a sample)
    -> int64 [samples][T]"""
    n = (len(off) - 1) // n_contigs
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n)]
    return all_counts(lists, flat, terms)


def brute_hit_set(per_list, genes):
    """H from the definition: every segment against every interval of every gene"""
    H = set()
    for g, seg in enumerate(per_list):
        for s, e in as_pairs(seg).tolist():
            if e <= s:
                continue
            for k, per in enumerate(genes):
                if any(a < e and s < b for a, b in as_pairs(per[g]).tolist() if b > a):
                    H.add(k)
    return H


def random_genes(r, n_genes, spans, max_len=40, per_gene=(1, 1, 2, 3)):
    """n_genes genes over groups of the given spans (0: no gene there): 1 to 3 intervals each, overlapping freely"""
    live = [g for g, span in enumerate(spans) if span > 1]
    genes = []
    for _ in range(n_genes):
        per = [[] for _ in spans]
        for _ in range(r.choice(per_gene)):
            g = r.choice(live)
            s = r.randrange(0, spans[g] - 1)
            per[g].append((s, min(spans[g], s + r.randint(1, max_len))))
        genes.append(per)
    return genes
