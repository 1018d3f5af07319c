#!/usr/bin/env python3
"""gat-reldist.py - do the segments sit closer to, or further from, an annotation's features than chance? on an MI355X
======================================================================================================================

The relative distance test (bedtools reldist, GenometriCorr): for each segment, the two features of the annotation that flank
its midpoint, and how far it sits from the nearer one as a fraction of the gap between them.  If segments and features ignore
each other that fraction is spread evenly over [0, 0.5]; mass near 0 means attraction, mass near 0.5 avoidance.  It works where
overlap fails -- features that are points, or sparse -- and does not confound association with feature density, as an absolute
distance does.  bedtools prints only the histogram and GenometriCorr tests it against a uniform null; here every value gets
gat-run.py's test against the sampler's null, which holds inside a fragmented workspace, with isochores and with clustered
segments.

   python gat-reldist.py --segments=segments.bed.gz --workspace=workspace.bed.gz --annotations=annotations.bed.gz
                         [--isochores=...] [--sampler=annotator] [--num-samples=1000] [--random-seed=N]
                         [--annotation-point=midpoint] [--bins=50]

The inputs are read and prepared as gat-run.py does; an annotation's intervals (normalized, taken to contig level) give one
reference point each: --annotation-point=midpoint (start + (end - start) // 2), start, or end (the last base, end - 1).  A
segment stands for its midpoint m; with p <= m < p' the flanking points it is inside and its relative distance is
min(m - p, p' - m) / (p' - p); a segment without two flanking points is outside.  --bins rows per (track, annotation with two
points on some contig), zeros included, then three summary rows whose `bin` is area, inside and outside:

   track annotation bin reldist_start reldist_end observed expected stddev fold l2fold pvalue qvalue samples_with_hit points

bin b covers the relative distances [reldist_start, reldist_end), 0.5 itself in the last bin; observed / expected: segments;
area: the area between the ECDF of the inside segments over the bins and the uniform one, 0 .. 1 (the test of the whole shape);
pvalue: gat-run.py's empirical two-sided p-value; qvalue: --qvalue-method (BH, bonferroni, holm, hommel, hochberg, BY, none) per
segment track, over the bin rows and separately over the area rows (inside and outside: 1); samples_with_hit: the samples
with a value above 0; points: the points of the annotation.  The null is reduced on the GPU where the sampler leaves its
lists (gat_amd/reldist.py): no sampled list comes back.  --descriptions is not offered.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import gat_amd as gat  # noqa: E402
from gat_amd import enrichment, reldist as Reldist  # noqa: E402


def buildParser(usage=None):
    """gat-run.py's parser without its counters and descriptions; --qvalue-method is limited to the adjustments of p-values,
    and the point of an interval and the number of bins"""
    parser = gat.buildParser(usage=usage, samplers=gat.TOOL_SAMPLERS + gat.UNIVERSE_SAMPLERS)
    for name in ("--counter", "--qvalue-method", "--descriptions"):
        parser.remove_option(name)
    parser.add_option("--annotation-point", dest="annotation_point", type="choice", choices=Reldist.ANNOTATION_POINTS,
                      help="the point of an annotation interval that is its reference point [default=%default]")
    parser.add_option("--bins", dest="bins", type="int", help="bins over the relative distances [0, 0.5] [default=%default]")
    parser.add_option("-q", "--qvalue-method", dest="qvalue_method", type="choice", choices=Reldist.QVALUE_METHODS,
                      help="multiple-testing correction per segment track, over the bin rows and over the area rows [default=%default]")
    parser.set_defaults(qvalue_method="BH", annotation_point="midpoint", bins=Reldist.BINS)
    return parser


def main(argv=None):
    argv = argv or sys.argv
    options, args = buildParser(usage=__doc__).parse_args(argv[1:])
    Reldist.check_options(options)

    def run(options, log):
        segments, annotations, workspace, sampler = enrichment.read_inputs(options)
        return Reldist.run(segments, annotations, workspace, sampler, options.num_samples, n_bins=options.bins,
                           annotation_point=options.annotation_point, random_seed=options.random_seed,
                           pseudo_count=options.pseudo_count, qvalue_method=options.qvalue_method)
    return enrichment.main(Reldist, argv, options, run)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
