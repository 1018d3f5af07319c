#!/usr/bin/env python3
"""gat-pairs.py - which annotations do the segments hit together more often than expected? on an MI355X
========================================================================================================

gat-run.py tests every annotation on its own.  This is the question about combinations: are the segments found where
annotation A and annotation B are both present more often than a random placement would put them there?  Every pair of
annotation tracks gets gat-run.py's test of the number of segments that share a base with both tracks, against the same
number for every sampled segment list -- the null model knows how the tracks overlap each other; the product of two marginal
expectations does not.

   python gat-pairs.py --segments=segments.bed.gz --workspace=workspace.bed.gz --annotations=annotations.bed.gz
                       [--isochores=...] [--sampler=annotator] [--num-samples=1000] [--random-seed=N] [--include-single]

The inputs are read and prepared as gat-run.py does.  One row per (track, annotation_a, annotation_b) that holds an observed
or a sampled hit:

   track annotation_a annotation_b observed expected stddev fold l2fold pvalue qvalue samples_with_hit observed_a observed_b

observed / expected: segments that hit both tracks; observed_a / observed_b: segments that hit the one track; pvalue:
gat-run.py's empirical two-sided p-value; qvalue: --qvalue-method (BH, bonferroni, holm, hommel, hochberg, BY, none) over the
rows written, per segment track; samples_with_hit: the samples with a segment that hits both.  --include-single adds a row
per annotation on its own (annotation_b == annotation_a).  The null is reduced on the GPU where the sampler leaves its lists
(gat_amd/pairs.py): no sampled list comes back.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import gat_amd as gat  # noqa: E402
from gat_amd import enrichment, pairs as Pairs  # noqa: E402


def buildParser(usage=None):
    """gat-run.py's parser without its counters, --qvalue-method limited to the adjustments of p-values, and --include-single"""
    parser = gat.buildParser(usage=usage, samplers=gat.TOOL_SAMPLERS + gat.UNIVERSE_SAMPLERS)
    parser.remove_option("--counter")
    parser.remove_option("--qvalue-method")
    parser.add_option("-q", "--qvalue-method", dest="qvalue_method", type="choice", choices=Pairs.QVALUE_METHODS,
                      help="multiple-testing correction of the rows written, per segment track [default=%default]")
    parser.add_option("--include-single", dest="include_single", action="store_true",
                      help="also write a row per annotation on its own (annotation_b == annotation_a) [default=%default]")
    parser.set_defaults(qvalue_method="BH", include_single=False)
    return parser


def main(argv=None):
    argv = argv or sys.argv
    options, args = buildParser(usage=__doc__).parse_args(argv[1:])
    Pairs.check_options(options)

    def run(options, log):
        segments, annotations, workspace, sampler = enrichment.read_inputs(options)
        return Pairs.run(segments, annotations, workspace, sampler, options.num_samples, random_seed=options.random_seed,
                         pseudo_count=options.pseudo_count, qvalue_method=options.qvalue_method,
                         include_single=options.include_single)
    return enrichment.main(Pairs, argv, options, run)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
