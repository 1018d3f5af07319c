#!/usr/bin/env python3
"""gat-metagene.py - how are the segments distributed along scaled features and their flanks? on an MI355X
=========================================================================================================

The metagene, or scaled-region profile: every feature (gene, enhancer, CpG island, TAD) is stretched to the same number of
body bins, 5' to 3', with flank bins of a fixed size on both sides.  Do the segments sit in the first tenth of gene bodies,
pile up at the 3' end, or avoid the body and prefer the flanks?  Every (feature track, bin) gets gat-run.py's test: the bases
of the segments in the bin, summed over the features, against the same number for every sampled segment list.  The null comes
from the sampler because the bins of long genes hold more bases, genes cluster in GC-rich isochores and overlapping genes count
a base twice.

   python gat-metagene.py --segments=segments.bed.gz --workspace=workspace.bed.gz --features=genes.bed.gz
                          [--isochores=...] [--sampler=annotator] [--num-samples=1000] [--random-seed=N]
                          [--body-bins=50] [--flank-bins=20] [--flank-bin-size=100] [--min-feature-length=BODY_BINS]
                          [--ignore-strand] [--profile-of=bases]

--features (alias --annotations): BED files; the segments and the workspace are prepared from them as gat-run.py prepares
them from its annotations, and the workspace options that refer to the annotations keep their meaning.  The features
themselves are read with their strand: column 6 `-` is the minus strand, anything else (or fewer than six columns) plus;
tracks are named by a `track name=` line, else column 4, else the file; --annotations-label pools everything.  Repeated (track,
contig, start, end, strand) are one feature; features overlap and nest and are neither merged nor cut to the workspace -- a
feature just outside still has a flank inside; features on contigs the workspace lacks are dropped; features shorter than
--min-feature-length (default: --body-bins, below which a body bin holds no base) are dropped and counted in the log.
--profile-of=midpoints counts the segments' midpoints instead of their bases.  2 x --flank-bins + --body-bins rows per (track,
feature track with a feature left), zeros included -- a metagene is plotted whole:

   track annotation bin region rel_start rel_end observed expected stddev fold l2fold pvalue qvalue samples_with_overlap features

region: upstream, body or downstream, by the feature's strand.  A flank bin covers the bases [rel_start, rel_end) from the
feature's 5' end (upstream: negative) or from its 3' end; a body bin the fractions [rel_start, rel_end) of the feature.
observed / expected: bases (or midpoints), a base counting once per feature whose window holds it; pvalue: gat-run.py's
empirical two-sided p-value; qvalue: --qvalue-method (BH, bonferroni, holm, hommel, hochberg, BY, none) over the rows written,
per segment track; samples_with_overlap: the samples with a base in the bin; features: the features of the track.  The null is
reduced on the GPU where the sampler leaves its lists (gat_amd/metagene.py): no sampled list comes back.  --descriptions is not
offered.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import gat_amd as gat  # noqa: E402
from gat_amd import enrichment, metagene as Metagene  # noqa: E402


def buildParser(usage=None):
    """gat-run.py's parser without its counters and descriptions; --features names the feature files, --qvalue-method is limited
    to the adjustments of p-values, and the geometry of the metagene"""
    parser = gat.buildParser(usage=usage, samplers=gat.TOOL_SAMPLERS + gat.UNIVERSE_SAMPLERS)
    for name in ("--counter", "--qvalue-method", "--descriptions"):
        parser.remove_option(name)
    parser.add_option("--features", dest="annotation_files", type="string", action="append",
                      help="BED file with the features, the strand in the sixth column (alias of --annotations)")
    parser.add_option("--ignore-strand", dest="ignore_strand", action="store_true", help="every feature is on the plus strand")
    parser.add_option("--body-bins", dest="body_bins", type="int", help="bins a feature's body is scaled to [default=%default]")
    parser.add_option("--flank-bins", dest="flank_bins", type="int", help="bins to either side of a feature [default=%default]")
    parser.add_option("--flank-bin-size", dest="flank_bin_size", type="int", help="bases per flank bin [default=%default]")
    parser.add_option("--min-feature-length", dest="min_feature_length", type="int",
                      help="features shorter than this are dropped [default: --body-bins]")
    parser.add_option("--profile-of", dest="profile_of", type="choice", choices=Metagene.PROFILES_OF,
                      help="what is counted: the segments' bases or their midpoints [default=%default]")
    parser.add_option("-q", "--qvalue-method", dest="qvalue_method", type="choice", choices=Metagene.QVALUE_METHODS,
                      help="multiple-testing correction of the rows written, per segment track [default=%default]")
    parser.set_defaults(qvalue_method="BH", ignore_strand=False, body_bins=Metagene.BODY_BINS, flank_bins=Metagene.FLANK_BINS,
                        flank_bin_size=Metagene.FLANK_BIN_SIZE, min_feature_length=None, profile_of="bases")
    return parser


def main(argv=None):
    argv = argv or sys.argv
    options, args = buildParser(usage=__doc__).parse_args(argv[1:])
    Metagene.check_options(options)

    def run(options, log):
        segments, annotations, workspace, sampler = enrichment.read_inputs(options)
        features = Metagene.read_features(options.annotation_files, Metagene.min_feature_length(options), options.ignore_strand,
                                          options.annotations_label, log)
        return Metagene.run(segments, features, workspace, sampler, options.num_samples, body_bins=options.body_bins,
                            flank_bins=options.flank_bins, flank_bin_size=options.flank_bin_size, profile_of=options.profile_of,
                            random_seed=options.random_seed, pseudo_count=options.pseudo_count, qvalue_method=options.qvalue_method)
    return enrichment.main(Metagene, argv, options, run)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
