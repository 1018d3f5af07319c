#!/usr/bin/env python3
"""gat-profile.py - how are the segments distributed around a class of points? on an MI355X
==========================================================================================

The most common question asked of a peak set: how do the segments lie around transcription start sites, motif centres or
exon ends -- upstream or downstream, how far does the enrichment reach, and is it shaped differently from chance?  Every anchor
track gets the aggregate profile of the segments around its anchors, 2 x --half-bins offset bins of --bin-size bases, and every
(anchor track, bin) gets gat-run.py's test: the bases of the segments in the bin, summed over the anchors, against the same
number for every sampled segment list.  The null comes from the sampler because anchors cluster and sit in gene-dense,
GC-rich isochores.

   python gat-profile.py --segments=segments.bed.gz --workspace=workspace.bed.gz --anchors=tss.bed.gz
                         [--isochores=...] [--sampler=annotator] [--num-samples=1000] [--random-seed=N]
                         [--anchor-point=five-prime] [--ignore-strand] [--bin-size=100] [--half-bins=50] [--profile-of=bases]

--anchors (alias --annotations): BED files; the segments and the workspace are prepared from them as gat-run.py prepares
them from its annotations, and the workspace options that refer to the annotations keep their meaning.  The anchors themselves
are read with their strand: column 6 `-` is the minus strand, anything else (or fewer than six columns) plus; tracks are named
by a `track name=` line, else column 4, else the file; --annotations-label pools everything.  --anchor-point: five-prime
(plus: start; minus: end - 1), three-prime (its mirror) or midpoint.  Repeated (track, contig, position, strand) are one anchor;
anchors are not cut to the workspace -- an anchor just outside still has a window inside; anchors on contigs the workspace
lacks are dropped.  The offset of a base x from the anchor (a, strand) is strand * (x - a): negative offsets are upstream.
--profile-of=midpoints counts the segments' midpoints instead of their bases.  2 x --half-bins rows per (track, anchor track
with an anchor left), zeros included -- a profile is plotted whole:

   track annotation bin offset_start offset_end observed expected stddev fold l2fold pvalue qvalue samples_with_overlap anchors

bin b covers the offsets [offset_start, offset_end); observed / expected: bases (or midpoints), a base counting once per
anchor whose window holds it; pvalue: gat-run.py's empirical two-sided p-value; qvalue: --qvalue-method (BH, bonferroni, holm,
hommel, hochberg, BY, none) over the rows written, per segment track; samples_with_overlap: the samples with a base in the bin;
anchors: the anchors of the track.  The null is reduced on the GPU where the sampler leaves its lists (gat_amd/profile.py): no
sampled list comes back.  --descriptions is not offered.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import gat_amd as gat  # noqa: E402
from gat_amd import enrichment, profile as Profile  # noqa: E402


def buildParser(usage=None):
    """gat-run.py's parser without its counters and descriptions; --anchors names the anchor files, --qvalue-method is limited
    to the adjustments of p-values, and the geometry of the profile"""
    parser = gat.buildParser(usage=usage, samplers=gat.TOOL_SAMPLERS + gat.UNIVERSE_SAMPLERS)
    for name in ("--counter", "--qvalue-method", "--descriptions"):
        parser.remove_option(name)
    parser.add_option("--anchors", dest="annotation_files", type="string", action="append",
                      help="BED file with the anchors, the strand in the sixth column (alias of --annotations)")
    parser.add_option("--anchor-point", dest="anchor_point", type="choice", choices=Profile.ANCHOR_POINTS,
                      help="the point of an interval that is its anchor [default=%default]")
    parser.add_option("--ignore-strand", dest="ignore_strand", action="store_true", help="every anchor is on the plus strand")
    parser.add_option("--bin-size", dest="bin_size", type="int", help="bases per offset bin [default=%default]")
    parser.add_option("--half-bins", dest="half_bins", type="int", help="bins to either side of an anchor [default=%default]")
    parser.add_option("--profile-of", dest="profile_of", type="choice", choices=Profile.PROFILES_OF,
                      help="what is counted: the segments' bases or their midpoints [default=%default]")
    parser.add_option("-q", "--qvalue-method", dest="qvalue_method", type="choice", choices=Profile.QVALUE_METHODS,
                      help="multiple-testing correction of the rows written, per segment track [default=%default]")
    parser.set_defaults(qvalue_method="BH", anchor_point="five-prime", ignore_strand=False, bin_size=Profile.BIN_SIZE,
                        half_bins=Profile.HALF_BINS, profile_of="bases")
    return parser


def main(argv=None):
    argv = argv or sys.argv
    options, args = buildParser(usage=__doc__).parse_args(argv[1:])
    Profile.check_options(options)

    def run(options, log):
        segments, annotations, workspace, sampler = enrichment.read_inputs(options)
        anchors = Profile.read_anchors(options.annotation_files, options.anchor_point, options.ignore_strand, options.annotations_label)
        return Profile.run(segments, anchors, workspace, sampler, options.num_samples, bin_size=options.bin_size,
                           half_bins=options.half_bins, profile_of=options.profile_of, random_seed=options.random_seed,
                           pseudo_count=options.pseudo_count, qvalue_method=options.qvalue_method)
    return enrichment.main(Profile, argv, options, run)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
