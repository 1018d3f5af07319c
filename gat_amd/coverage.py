"""gat-coverage: where a null model puts its segments.

Per-bin coverage of the sampled segments -- bases, segment starts and segment ends per bin, summed over the samples --
for one segment track in its workspace: what computeSegmentDensityProfile of the reference's validation material
(test/validate_randomization.py:212-247; the figures of doc/testingPosition.rst and doc/simulators.rst) draws from 100
samples of toy workspaces with per-base Python loops.  Here the samples are binned on the device where the sampler leaves
them (k_coverage, gat_sample_coverage): no list comes back to the host.

Bin b of a contig is [b * bin_size, (b + 1) * bin_size); a contig has ceil(largest workspace end / bin_size) bins.  The
reference clamps every sampled segment to [0, workspace.max()); here the sampled bases beyond the last bin are reported
per contig (`outside`) -- samplers that leave the workspace (shift, the permutations) show there.

Under an initialised torch.distributed process group the call runs on the calling rank's device, all samples, without
sharding: every rank that calls it computes the whole profile.
"""
import collections

import numpy as np

from . import problem
from .engine import SAMPLER_CLASSES as SAMPLERS
from .engine import check_sampler, get_context, sampler_from_options


class Coverage(object):
    """the profile of one segment track: `contigs` (the workspace's, sampled ones first), `bin_size`, `num_samples`, and per
    contig int64 arrays of its bins -- bases / starts / ends: the samples' sums; workspace_bases / segment_bases: the bases
    of the workspace and of the input segments in each bin -- and outside[contig], the sampled bases beyond the last bin."""

    def __init__(self, contigs, bin_size, num_samples):
        self.contigs, self.bin_size, self.num_samples = list(contigs), int(bin_size), int(num_samples)
        self.bases, self.starts, self.ends, self.outside = {}, {}, {}, {}
        self.workspace_bases, self.segment_bases = {}, {}
        self.stats = None

    def n_bins(self, contig):
        return len(self.bases[contig])


def bin_bases(a, bin_size, n_bins):
    """bases of the segments of a SEG array in each of n_bins bins of bin_size (int64; any list: overlaps count twice)"""
    edges = np.arange(n_bins + 1, dtype=np.int64) * int(bin_size)
    if len(a) == 0:
        return np.zeros(n_bins, dtype=np.int64)

    def below(x):                                        # sum over the list of min(x, edge), for every edge
        x = np.sort(x.astype(np.int64))
        run = np.concatenate([[0], np.cumsum(x)])
        k = np.searchsorted(x, edges, side="right")
        return run[k] + edges * (len(x) - k)

    cum = below(a["end"]) - below(a["start"])
    return np.diff(cum)


def flatten(segs, workspace, sampler):
    """the flat problem of a track (gat_problem_desc) as sample_counts builds it, without annotation tracks: gat_problem_create
    takes none, and the coverage needs none."""
    sa, wa = segs.asArrays(), workspace.asArrays()
    flat = problem.flatten_units(sa, wa, [], getattr(sampler, "bucket_size", 0), getattr(sampler, "nbuckets", 100000))
    flat.update(sampler.flat_fields())
    return flat, sa, wa


def sample_coverage(segs, workspace, sampler, num_samples, bin_size, random_seed=None, ctx=None):
    """Coverage of num_samples samples of `segs` in `workspace` (IntervalDictionary, isochore level, as sample_counts takes
    them) under `sampler`.  random_seed: base of the per-unit streams (None: drawn from numpy's global RandomState)."""
    from . import _lib
    check_sampler(sampler)
    bin_size, num_samples = int(bin_size), int(num_samples)
    if not 1 <= bin_size <= 2 ** 31:
        raise ValueError("bin_size %d outside [1, 2^31]" % bin_size)
    if num_samples < 0:
        raise ValueError("num_samples < 0")
    seed = int(np.random.randint(0, 2 ** 32)) if random_seed is None else int(random_seed)
    flat, sa, wa = flatten(segs, workspace, sampler)
    contig_ws = problem.from_isochores(wa)
    contig_segs = problem.from_isochores(sa)
    sampled = list(flat["contig_names"])
    contigs = sampled + [c for c in contig_ws if c not in set(sampled)]
    n_bins = collections.OrderedDict()
    for c in contigs:
        w = contig_ws.get(c)
        top = int(w["end"].max()) if w is not None and len(w) else 0
        n_bins[c] = (top + bin_size - 1) // bin_size
    out = Coverage(contigs, bin_size, num_samples)
    for c in contigs:
        out.workspace_bases[c] = bin_bases(contig_ws.get(c, ()), bin_size, n_bins[c])
        out.segment_bases[c] = bin_bases(contig_segs.get(c, ()), bin_size, n_bins[c])
        out.bases[c], out.starts[c], out.ends[c] = (np.zeros(n_bins[c], dtype=np.int64) for _ in range(3))
        out.outside[c] = 0
    if not sampled or num_samples == 0:
        return out
    ctx = ctx or get_context()
    P = _lib.Problem(ctx, flat)
    try:
        bases, starts, ends, outside, off = P.sample_coverage(seed, 0, num_samples, bin_size, [n_bins[c] for c in sampled])
        out.stats = P.last_stats
    finally:
        P.close()
    for k, c in enumerate(sampled):
        out.bases[c], out.starts[c], out.ends[c] = (x[off[k]:off[k + 1]].copy() for x in (bases, starts, ends))
        out.outside[c] = int(outside[k])
    return out


HEADER = ("track", "contig", "start", "end", "workspace_bases", "segment_bases", "sampled_bases", "starts", "ends", "depth")


def write_rows(outfile, track, cov):
    """one row per bin that holds a workspace base or a sampled base; a `# track contig outside_bases` line per contig with
    sampled bases beyond its last bin.  depth = sampled_bases / (num_samples * (end - start))."""
    for c in cov.contigs:
        keep = np.flatnonzero((cov.workspace_bases[c] > 0) | (cov.bases[c] > 0))
        for b in keep.tolist():
            start, end = b * cov.bin_size, (b + 1) * cov.bin_size
            sampled = int(cov.bases[c][b])
            depth = sampled / (cov.num_samples * (end - start)) if cov.num_samples else 0.0
            outfile.write("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%r\n" % (
                track, c, start, end, cov.workspace_bases[c][b], cov.segment_bases[c][b], sampled, cov.starts[c][b], cov.ends[c][b], depth))
        if cov.outside[c]:
            outfile.write("# %s\t%s\t%d\n" % (track, c, cov.outside[c]))


def build_inputs(options):
    """segment tracks and the workspace of a run as gat-run.py prepares them (IO.buildSegments / IO.applyIsochores,
    gat/IO.py:88-293) with the steps that concern annotations left out: none are read.  Returns (segments, workspace):
    an IntervalCollection at isochore level and the collapsed workspace's IntervalDictionary."""
    from . import io as IO
    from . import engine
    for attr, what in (("segment_files", "segment"), ("workspace_files", "workspace")):
        setattr(options, attr, IO.expandGlobs(getattr(options, attr)))
        if not getattr(options, attr):
            raise ValueError("please specify at least one %s file" % what)
    segments = IO.readSegmentList("segments", options.segment_files, ignore_tracks=options.ignore_segment_tracks)
    segments.normalize()
    if segments.sum() == 0:
        raise ValueError("segments file is empty - run aborted")
    workspaces = IO.readSegmentList("workspaces", options.workspace_files)
    workspaces.normalize()
    workspaces.collapse()
    workspaces.restrict("collapsed")
    if options.isochore_files:
        isochores = engine.IntervalCollection(name="isochores")
        isochores.intervals = IO.readFromBed(IO.expandGlobs(options.isochore_files))
        for step in (isochores.sort, isochores.check, isochores.normalize):
            step()
        isochores.intersect(workspaces["collapsed"])
        workspaces.toIsochores(isochores, truncate=True)
        segments.toIsochores(isochores, truncate=False)
        for coll, what in ((workspaces, "workspaces"), (segments, "segments")):
            if coll.sum() == 0:
                raise ValueError("isochores and %s do not overlap" % what)
    else:
        segments.filter(workspaces["collapsed"])
    return segments, workspaces["collapsed"]


def make_sampler(options):
    """the sampler of --sampler, built as gat.fromSegments builds it (scripts/gat-run.py:129-140 of the reference)"""
    return sampler_from_options(options)
