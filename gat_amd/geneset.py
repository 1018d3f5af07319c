"""gat-geneset: do the segments hit the genes of a gene set (a GO term, a pathway) more often than chance would have it?

The reference's gat-geneset.py answers with a hypergeometric draw -- "the segments hit n of N genes; K genes carry term t; k of
the hit genes carry it" -- which takes every gene to be hit equally often.  Genes are not: long genes, genes in gene-poor
isochores and clustered families are hit far more often by segments placed at random (the bias GREAT was written about).  The
null that knows this is the one this project samples.  Here every term gets gat-run's test of

    c = the genes of the term that share a base with a segment

against the same count of every sampled segment list.  The genes are flattened on the host into disjoint pieces, each with the
genes that cover it (flatten_genes); the device finds the pieces a segment reaches with one search per segment, marks the genes
in a bitmap per list and counts every term from the bitmap (k_geneset_hits, k_geneset_terms: gat_sample_geneset_enrichment).
The (samples x terms) matrix is never formed: five integers per term come back -- n_pos, sum, sumsq, n_less, n_eq;
include/gat_mi355.h has the definition -- and the row's statistics are made from those with enrichment.bin_statistics.  A pseudo-term
of all genes rides along in every call: its words are the null of n = the genes hit at all.  The hypergeometric columns of the
reference are written beside the sampled ones, so that the bias the sampled null removes can be seen.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding.
"""
import collections
import math

import numpy as np

from . import enrichment
from . import intervals as iv
from . import problem
from .engine import AnnotatorResult, get_context

TOOL = "gat-geneset"
WORDS, QVALUE_METHODS, bin_statistics = enrichment.WORDS, enrichment.QVALUE_METHODS, enrichment.bin_statistics
flatten, make_sampler, build_inputs = enrichment.flatten, enrichment.make_sampler, enrichment.build_inputs
MAX_GENES = 262144                        # genes of one call (GAT_GENESET_MAX_GENES)
HEADER = ("track", "annotation", "genes_in_workspace", "genes_with_annotation", "genes_with_segments",
          "genes_with_annotation_and_segments", "expected", "fold", "pvalue", "qvalue", "stddev", "l2fold", "samples_with_hit",
          "expected_genes_with_segments", "hypergeom_expected", "hypergeom_fold", "hypergeom_pvalue")
ORDERS = ("track", "annotation", "fold", "pvalue", "qvalue", "observed")


# ---- the genes ----------------------------------------------------------------------------------------------------------------------------
def flatten_genes(genes, contigs):
    """genes[g]: dict contig -> intervals (SEG array or pairs) of gene g, in any order, overlapping or not; a gene's own
    intervals are merged first.  Returns (pieces, piece_off, member_off, members) as gat_list_geneset_hits takes them, the
    groups being `contigs` in their order: per contig the elementary intervals between consecutive gene boundaries that a gene
    covers -- sorted, disjoint, none empty, adjacent ones apart -- and per piece the ascending ids of the genes that cover it."""
    pieces, counts, members = [], [], []
    piece_off = np.zeros(len(contigs) + 1, dtype=np.int64)
    for c, contig in enumerate(contigs):
        start, end, gene = [], [], []
        for g, per in enumerate(genes):
            if contig in per and len(per[contig]):
                a = iv.merge(iv.as_segments(per[contig]), 0)
                start.append(a["start"].astype(np.int64))
                end.append(a["end"].astype(np.int64))
                gene.append(np.full(len(a), g, dtype=np.int64))
        if not start:
            piece_off[c + 1] = piece_off[c]
            continue
        start, end, gene = np.concatenate(start), np.concatenate(end), np.concatenate(gene)
        bounds = np.unique(np.concatenate([start, end]))
        lo, hi = np.searchsorted(bounds, start), np.searchsorted(bounds, end)
        cnt = hi - lo                                                    # elementary intervals an interval covers
        first = np.repeat(np.cumsum(cnt) - cnt, cnt)
        elem = np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - first)
        who = np.repeat(gene, cnt)
        order = np.lexsort((who, elem))
        elem, who = elem[order], who[order]
        covered, per_piece = np.unique(elem, return_counts=True)
        pieces.append(iv.make(bounds[covered], bounds[covered + 1]))
        counts.append(per_piece)
        members.append(who)
        piece_off[c + 1] = piece_off[c] + len(covered)
    member_off = np.zeros(int(piece_off[-1]) + 1, dtype=np.int64)
    if counts:
        np.cumsum(np.concatenate(counts), out=member_off[1:])
    return (np.concatenate(pieces) if pieces else iv.EMPTY.copy(), piece_off, member_off,
            np.concatenate(members).astype(np.int32) if members else np.zeros(0, dtype=np.int32))


def gene_table(annotations):
    """the genes of a run: `annotations` is the gene file read as an annotation collection -- a BED of four columns and more,
    the fourth the gene id, lines with the same id one gene -- after it went through the workspace and the isochores like any
    annotation track.  Returns (ids, genes, dropped): genes[g] the dict contig -> SEG array (contig level) of gene ids[g], in
    the file's order; genes left with no base are dropped and counted."""
    ids, genes, dropped = [], [], 0
    for name in annotations.tracks:
        per = collections.OrderedDict((c, a) for c, a in problem.from_isochores(annotations[name].asArrays()).items() if len(a))
        if per:
            ids.append(name)
            genes.append(per)
        else:
            dropped += 1
    return ids, genes, dropped


# ---- the map ------------------------------------------------------------------------------------------------------------------------------
def read_gene_sets(filename):
    """the map file: two tab-separated columns, gene then term, after one header line; `#` lines are comments; n:n; a repeated
    line counts once.  Returns an OrderedDict term -> [gene ids], terms and genes in the order of their first line."""
    from . import io as IO
    out = collections.OrderedDict()
    seen = set()
    header = True
    with IO.openFile(filename, "r") as infile:
        for line in infile:
            if line.startswith("#") or not line.strip():
                continue
            if header:
                header = False
                continue
            fields = line.rstrip("\n").split("\t")
            if len(fields) < 2:
                raise IOError("malformatted entry in %s: %r (gene<TAB>term)" % (filename, line))
            gene, term = fields[0], fields[1]
            if (gene, term) not in seen:
                seen.add((gene, term))
                out.setdefault(term, []).append(gene)
    return out


def term_table(gene_sets, ids):
    """the terms as gat_list_geneset_hits takes them: gene_sets an OrderedDict term -> gene ids (read_gene_sets), ids the
    genes kept (gene_table).  Returns (terms, term_off, term_genes, unknown): every term of the map in its order, empty ones
    too; gene ids the gene file lacks are ignored and counted (each id once)."""
    index = dict((g, k) for k, g in enumerate(ids))
    terms, lists, unknown = [], [], set()
    for term, members in gene_sets.items():
        unknown.update(g for g in members if g not in index)
        terms.append(term)
        lists.append(np.unique(np.array([index[g] for g in members if g in index], dtype=np.int32)))
    term_off = np.zeros(len(terms) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=term_off[1:])
    return terms, term_off, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32), len(unknown)


def with_all_genes(term_off, term_genes, n_genes):
    """the terms and behind them the pseudo-term of all genes: its count is n = |H|, the genes hit at all"""
    return (np.append(term_off, term_off[-1] + n_genes).astype(np.int64),
            np.concatenate([term_genes, np.arange(n_genes, dtype=np.int32)]).astype(np.int32))


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
def hypergeometric(k, N, K, n):
    """(expected, fold, pvalue) of the reference's gat-geneset.py: nK/N, k / expected and P(X >= k) of a draw of n from N with
    K marked; 0, 1.0 and 1.0 when n, N or K is 0"""
    k, N, K, n = int(k), int(N), int(K), int(n)
    if n == 0 or N == 0 or K == 0:
        return 0, 1.0, 1.0
    import scipy.stats
    expected = float(n * K) / N
    return expected, k / expected, float(scipy.stats.hypergeom.sf(k - 1, N, K, n))


class GenesetResult(object):
    """a row of the table: one (segment track, term)"""
    format_observed = AnnotatorResult.format_observed
    format_expected = AnnotatorResult.format_expected
    format_fold = AnnotatorResult.format_fold
    format_pvalue = AnnotatorResult.format_pvalue
    headers = list(HEADER)

    def __init__(self, track, annotation, genes_in_workspace, genes_with_annotation, genes_with_segments, observed, words,
                 all_words, num_samples, pseudo_count=1.0, position=0):
        self.track, self.annotation = track, annotation
        self.genes_in_workspace, self.genes_with_annotation = int(genes_in_workspace), int(genes_with_annotation)
        self.genes_with_segments, self.observed, self.nsamples = int(genes_with_segments), int(observed), int(num_samples)
        self.words = tuple(int(w) for w in words)
        self.samples_with_hit = self.words[0]
        self.expected, self.stddev, self.fold, self.pvalue = bin_statistics(observed, words, num_samples, pseudo_count)
        self.expected_genes_with_segments = int(all_words[1]) / int(num_samples)
        self.hypergeom_expected, self.hypergeom_fold, self.hypergeom_pvalue = hypergeometric(
            self.observed, self.genes_in_workspace, self.genes_with_annotation, self.genes_with_segments)
        self.qvalue = 1.0
        self.position = position              # (the term's index in the map's order)

    def __str__(self):
        logfold = self.format_fold % math.log(self.fold, 2) if self.fold > 0 else "-inf"
        return "\t".join((self.track, self.annotation, "%i" % self.genes_in_workspace, "%i" % self.genes_with_annotation,
                          "%i" % self.genes_with_segments, self.format_observed % self.observed,
                          self.format_expected % self.expected, self.format_fold % self.fold, self.format_pvalue % self.pvalue,
                          self.format_pvalue % self.qvalue, self.format_expected % self.stddev, logfold,
                          "%i" % self.samples_with_hit, self.format_expected % self.expected_genes_with_segments,
                          self.format_expected % self.hypergeom_expected, self.format_fold % self.hypergeom_fold,
                          self.format_pvalue % self.hypergeom_pvalue))


def rows(track, terms, term_off, n_genes, observed, words, num_samples, pseudo_count=1.0, min_term_genes=1):
    """the rows of one segment track: terms the names, term_off their CSR offsets (K = the difference), observed [T + 1] and
    words [T + 1][5] of the T terms and, last, of the pseudo-term of all genes.  One row per term with K >= min_term_genes, in
    the terms' order."""
    observed, words = np.asarray(observed, dtype=np.int64), np.asarray(words, dtype=np.int64)
    assert len(observed) == len(terms) + 1 and words.shape == (len(terms) + 1, len(WORDS))
    K = np.diff(np.asarray(term_off, dtype=np.int64))
    return [GenesetResult(track, a, n_genes, K[t], observed[-1], observed[t], words[t], words[-1], num_samples, pseudo_count, position=t)
            for t, a in enumerate(terms) if K[t] >= min_term_genes]


def set_qvalues(results, method="BH"):
    """q-values over the rows written, per segment track"""
    enrichment.set_qvalues(results, method, TOOL)


def check_options(options):
    """what gat-geneset does not do, refused before anything is read"""
    enrichment.check_options(options, TOOL, "a gene is an interval list, not a position")


def track_geneset(track, segs, ids, genes, terms, term_off, term_genes, workspace, sampler, num_samples, random_seed=None,
                  pseudo_count=1.0, min_term_genes=1, ctx=None):
    """the rows of one segment track: `segs` and `workspace` IntervalDictionaries at isochore level as sample_counts takes
    them; ids / genes from gene_table, terms / term_off / term_genes from term_table.  Returns (rows, the problem's unit count)."""
    from . import _lib
    if len(ids) > MAX_GENES:
        raise ValueError("gat-geneset: %d genes are more than %d" % (len(ids), MAX_GENES))
    num_samples, seed, flat, _, contigs, lists, list_off = enrichment.track_start(segs, workspace, sampler, num_samples, random_seed)
    if not contigs or not terms:
        return [], flat["n_units"]
    G, T = len(ids), len(terms) + 1
    pieces, piece_off, member_off, members = flatten_genes(genes, contigs)
    all_off, all_genes = with_all_genes(term_off, term_genes, G)
    ctx = ctx or get_context()
    observed = ctx.list_geneset_hits(lists, list_off, 1, pieces, piece_off, member_off, members, G, all_off, all_genes, T, len(contigs))[0]
    P = _lib.Problem(ctx, flat)
    try:
        words = P.sample_geneset_enrichment(seed, 0, num_samples, pieces, piece_off, member_off, members, G, all_off, all_genes, T, observed)
    finally:
        P.close()
    return rows(track, terms, term_off, G, observed, words, num_samples, pseudo_count, min_term_genes), flat["n_units"]


def run(segments, annotations, gene_sets, workspace, sampler, num_samples, random_seed=None, pseudo_count=1.0, qvalue_method="BH",
        min_term_genes=1, ctx=None, log=None):
    """every segment track against every term: the GenesetResults track by track.  annotations: the gene file as an annotation
    collection (gene_table); gene_sets: read_gene_sets' map.  random_seed: base of the per-unit streams (None: drawn from
    numpy's global RandomState); every track takes the next num_samples * n_units streams, as gat.run hands them out.  log: a
    callable that takes a line about the genes dropped and the ids ignored."""
    enrichment.check_qvalue_method(qvalue_method, TOOL)
    ids, genes, dropped = gene_table(annotations)
    terms, term_off, term_genes, unknown = term_table(gene_sets, ids)
    if log:
        log("gat-geneset: %d genes in the workspace, %d genes without a base in it dropped" % (len(ids), dropped))
        log("gat-geneset: %d terms, %d gene ids of the map not in the gene file ignored" % (len(terms), unknown))
    return enrichment.run_tracks(segments, lambda track, segs, seed: track_geneset(
        track, segs, ids, genes, terms, term_off, term_genes, workspace, sampler, num_samples, seed, pseudo_count, min_term_genes, ctx),
        num_samples, random_seed, qvalue_method, TOOL)


def write_results(outfile, results, order="track"):
    """the table, rows ordered by --order (ties in the terms' order)"""
    enrichment.write_results(outfile, results, HEADER, {"track": lambda x: (x.track, x.position), "annotation": lambda x: (x.position, x.track)}, order)
