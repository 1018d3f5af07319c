#!/usr/bin/env python3
"""gat-local.py - where along the genome do segments and an annotation overlap more than expected? on an MI355X
=============================================================================================================

gat-run.py gives one number per annotation: the overlap over the whole workspace.  This is the question that follows a
significant row -- one locus, one chromosome arm, or everywhere?  The genome is cut into bins of --bin-size bases and every
(annotation, bin) gets gat-run.py's test: the bases the segments share with the annotation inside the bin against the same
number for every sampled segment list.

   python gat-local.py --segments=segments.bed.gz --workspace=workspace.bed.gz --annotations=annotations.bed.gz
                       [--isochores=...] [--sampler=annotator] [--num-samples=1000] [--random-seed=N] [--bin-size=100000]

The inputs are read and prepared as gat-run.py does.  One row per (track, annotation, bin) that holds an observed or a sampled
base:

   track annotation contig start end observed expected stddev fold l2fold pvalue qvalue samples_with_overlap

observed / expected: bases; pvalue: gat-run.py's empirical two-sided p-value; qvalue: --qvalue-method (BH, bonferroni, holm,
hommel, hochberg, BY, none) over the rows written, per segment track; samples_with_overlap: the samples with a base in the
bin.  The null is reduced on the GPU where the sampler leaves its lists (gat_amd/local.py): no sampled list comes back.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import gat_amd as gat  # noqa: E402
from gat_amd import enrichment, local as Local  # noqa: E402


def buildParser(usage=None):
    """gat-run.py's parser without its counters, --qvalue-method limited to the adjustments of p-values, and --bin-size"""
    parser = gat.buildParser(usage=usage, samplers=gat.TOOL_SAMPLERS + gat.UNIVERSE_SAMPLERS)
    parser.remove_option("--counter")
    parser.remove_option("--qvalue-method")
    parser.add_option("-q", "--qvalue-method", dest="qvalue_method", type="choice", choices=Local.QVALUE_METHODS,
                      help="multiple-testing correction of the rows written, per segment track [default=%default]")
    parser.add_option("--bin-size", dest="bin_size", type="int", help="bases per bin [default=%default]")
    parser.set_defaults(bin_size=Local.BIN_SIZE, qvalue_method="BH")
    return parser


def main(argv=None):
    argv = argv or sys.argv
    options, args = buildParser(usage=__doc__).parse_args(argv[1:])
    Local.check_options(options)

    def run(options, log):
        segments, annotations, workspace, sampler = enrichment.read_inputs(options)
        return Local.run(segments, annotations, workspace, sampler, options.num_samples, bin_size=options.bin_size,
                         random_seed=options.random_seed, pseudo_count=options.pseudo_count, qvalue_method=options.qvalue_method)
    return enrichment.main(Local, argv, options, run)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
