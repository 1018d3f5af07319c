#!/usr/bin/env python3
"""gat-geneset.py - gene-set enrichment of the segments against the sampled null, on an MI355X
==============================================================================================

Do the segments hit the genes of a gene set -- a GO term, a pathway -- more often than a random placement would?  The
reference's gat-geneset.py tests with a hypergeometric draw, which takes every gene to be hit equally often; long genes and
genes in gene-poor regions are hit far more often by segments placed at random.  Here every term gets gat-run.py's test of the
number of its genes that share a base with a segment, against the same number for every sampled segment list.

   python gat-geneset.py --segments=segments.bed.gz --workspace=workspace.bed.gz --genes=genes.bed.gz --gene-sets=gene2term.tsv
                         [--isochores=...] [--sampler=annotator] [--num-samples=1000] [--random-seed=N] [--min-term-genes=1]

--genes (alias --annotations): a BED of four columns and more, the fourth the gene id; lines with the same id are one gene; the
genes are cut to the workspace like annotation tracks, and genes left with no base are dropped.  --gene-sets / -m: two
tab-separated columns, gene then term, after a header line; `#` lines are comments; n:n; ids the gene file lacks are ignored.
One row per (track, term) with at least --min-term-genes genes in the workspace:

   track annotation genes_in_workspace genes_with_annotation genes_with_segments genes_with_annotation_and_segments expected
   fold pvalue qvalue stddev l2fold samples_with_hit expected_genes_with_segments hypergeom_expected hypergeom_fold
   hypergeom_pvalue

The first ten columns are the reference's, now from the sampled null: expected is the mean over the samples of the term's genes
hit, pvalue gat-run.py's empirical one, qvalue --qvalue-method (BH, bonferroni, holm, hommel, hochberg, BY, none) over the rows
written, per segment track.  expected_genes_with_segments is the mean over the samples of the genes hit at all; the hypergeom_*
columns are the reference's test on the same counts.  The null is reduced on the GPU where the sampler leaves its lists
(gat_amd/geneset.py): no sampled list comes back.  --descriptions is not offered.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import gat_amd as gat  # noqa: E402
from gat_amd import enrichment, geneset as Geneset  # noqa: E402


def buildParser(usage=None):
    """gat-run.py's parser without its counters and descriptions; --genes names the gene file, -m goes from --sampler to
    --gene-sets as in the reference's script, --qvalue-method is limited to the adjustments of p-values, and --min-term-genes"""
    parser = gat.buildParser(usage=usage, samplers=gat.TOOL_SAMPLERS + gat.UNIVERSE_SAMPLERS)
    sampler = parser.get_option("--sampler")
    for name in ("--counter", "--qvalue-method", "--descriptions", "--sampler"):
        parser.remove_option(name)
    parser.add_option("--sampler", dest="sampler", type="choice", choices=sampler.choices, help="the sampler [default=%default]")
    parser.add_option("--genes", dest="annotation_files", type="string", action="append",
                      help="BED file with the genes, the gene id in the fourth column (alias of --annotations)")
    parser.add_option("-m", "--gene-sets", dest="gene_sets", type="string",
                      help="tab-separated file gene<TAB>term with a header line: which genes carry which term")
    parser.add_option("-q", "--qvalue-method", dest="qvalue_method", type="choice", choices=Geneset.QVALUE_METHODS,
                      help="multiple-testing correction of the rows written, per segment track [default=%default]")
    parser.add_option("--min-term-genes", dest="min_term_genes", type="int",
                      help="terms with fewer genes in the workspace are not tested [default=%default]")
    parser.set_defaults(qvalue_method="BH", min_term_genes=1, gene_sets=None)
    return parser


def main(argv=None):
    argv = argv or sys.argv
    options, args = buildParser(usage=__doc__).parse_args(argv[1:])
    Geneset.check_options(options)
    if not options.gene_sets:
        raise ValueError("please specify the gene sets (--gene-sets)")

    def run(options, log):
        gene_sets = Geneset.read_gene_sets(options.gene_sets)
        segments, annotations, workspace, sampler = enrichment.read_inputs(options)
        return Geneset.run(segments, annotations, gene_sets, workspace, sampler, options.num_samples, random_seed=options.random_seed,
                           pseudo_count=options.pseudo_count, qvalue_method=options.qvalue_method,
                           min_term_genes=options.min_term_genes, log=log)
    return enrichment.main(Geneset, argv, options, run)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
