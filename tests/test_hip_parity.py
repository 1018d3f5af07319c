"""GPU parity: the HIP path (through the C ABI) against the reference-generated goldens and the
CPU oracle on the same seeded inputs.  Bit-exact: integer counts, sampled segment lists, and
IEEE doubles for the density counter."""
import hashlib
import json
import os

import numpy as np
import pytest

from gat_amd import _lib, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = ["config1", "small_isochores", "small_contigs", "small_isochores_truncated", "config2_s12",
        "density_ungapped", "dense", "long_segments", "small_isochores_sampler_segments"]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _flat(z):
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", RUNS)
def test_golden_counts_and_samples(ctx, name):
    """count matrix and sampled lists == what the reference produced (per-unit stream contract)."""
    z = np.load(os.path.join(G, "run_%s.npz" % name))
    counters = [str(c) for c in z["counters"]]
    S = int(z["num_samples"])
    P = _lib.Problem(ctx, _flat(z))
    counts = P.sample_and_count(counters, int(z["seed"]), 0, S)
    want = z["counts_mode1"]
    for k, c in enumerate(counters):
        if c == "nucleotide-density":
            assert np.array_equal(counts[k], want[k]), c
        else:
            assert np.array_equal(counts[k].astype(np.float64), want[k]), c
    seg, off = P.sample(int(z["seed"]), 0, S)
    h = hashlib.sha256()
    for i in range(len(off) - 1):
        h.update(seg[off[i]:off[i + 1]].tobytes())
    assert h.hexdigest() == str(z["samples_sha256_mode1"])
    if "samples_mode1" in z.files:
        assert np.array_equal(off, z["samples_off_mode1"])
        assert np.array_equal(seg, z["samples_mode1"])
    P.close()


@pytest.mark.parametrize("name", ["config3_s4", "config5_s2", "config4_s2", "config3all_s3", "config2all_s4"])
def test_golden_config_shapes_against_the_reference(ctx, name):
    """configs 3, 5 and 4 at their full interval counts (100 tracks x 192 isochore units; density against a 1M-interval
    annotation; 100 k segments x 1 000 tracks; config 3 again with all six counters side by side): count matrices and sampled
    lists == what the REFERENCE's computeSample produced for the same inputs
    (tests/golden/make_goldens.py g9), and the one-stream mode == its gat.run."""
    from test_oracle_golden import config_golden
    z, flat = config_golden(name)
    counters = [str(c) for c in z["counters"]]
    S, seed = int(z["num_samples"]), int(z["seed"])
    P = _lib.Problem(ctx, flat)
    try:
        counts = P.sample_and_count(counters, seed, 0, S)
        for k, c in enumerate(counters):
            got = counts[k] if c == "nucleotide-density" else counts[k].astype(np.float64)
            assert np.array_equal(got, z["counts_mode1"][k]), (name, c)
        seg, off = P.sample(seed, 0, S)
        assert np.array_equal(np.diff(off), z["sample_list_lengths"])
        h = hashlib.sha256()
        for i in range(len(off) - 1):
            h.update(seg[off[i]:off[i + 1]].tobytes())
        assert h.hexdigest() == str(z["samples_sha256_mode1"])
        # the reference's real gat.run (one global stream): k_serial
        serial = P.sample_and_count_serial(counters, _lib.mt19937_seed(seed), S)
        for k, c in enumerate(counters):
            got = serial[k] if c == "nucleotide-density" else serial[k].astype(np.float64)
            assert np.array_equal(got, z["counts_mode0"][k]), (name, c, "mode 0")
    finally:
        P.close()


def _single_unit_flat(segments, workspace, bucket_size, nbuckets):
    s, w = O.segs(segments), O.segs(workspace)
    return dict(n_units=1, segs=s, seg_off=[0, len(s)], ws=w, ws_off=[0, len(w)], unit_contig=[0], n_contigs=1,
                merge_contigs=0, n_tracks=1, annos=w, anno_off=[0, len(w)], cws_nseg=[len(w)],
                bucket_size=bucket_size, nbuckets=nbuckets)


def test_golden_sampler_kats(ctx):
    """SamplerAnnotator.sample known answers taken from the reference (tests/golden/sampler.json)."""
    with open(os.path.join(G, "sampler.json")) as f:
        cases = json.load(f)
    nrun = 0
    for c in cases:
        flat = _single_unit_flat(c["segments"], c["workspace"], c["bucket_size"], c["nbuckets"])
        if "error" in c:
            with pytest.raises(ValueError):
                _lib.Problem(ctx, flat)
            continue
        P = _lib.Problem(ctx, flat)
        for run in c["runs"]:
            seg, off = P.sample(run["seed"], 0, 1)       # unit stream seed = seed + 0*1 + 0
            assert len(seg) == run["n"], (c["name"], run["seed"])
            assert hashlib.sha256(seg.tobytes()).hexdigest() == run["sha256"], (c["name"], run["seed"])
            nrun += 1
        P.close()
    assert nrun >= 250


def _random_problem(rs, n_contigs, n_segs, n_tracks, isochores, dense=False):
    contigs = dict(("c%d" % i, int(rs.randint(20000, 400000))) for i in range(n_contigs))
    import collections
    contigs = collections.OrderedDict(sorted(contigs.items()))
    segs = synthetic.random_segments(contigs, n_segs, 60 if not dense else 400, int(rs.randint(1 << 30)))
    annos = [("t%d" % t, synthetic.random_segments(contigs, int(rs.randint(20, 400)), int(rs.randint(50, 2000)),
                                                   int(rs.randint(1 << 30)))) for t in range(n_tracks)]
    ws = synthetic.workspace_ungapped(contigs, pieces=int(rs.randint(1, 5)), gap=2000)
    from gat_amd import problem
    iso = synthetic.isochores_blocks(contigs, nclasses=int(rs.randint(2, 4)), block=int(rs.randint(5000, 40000))) if isochores else None
    return problem.flatten_arrays(segs, annos, ws, iso)


SEGMENT_SIDE = ["nucleotide-overlap", "nucleotide-density", "segment-overlap", "segment-midoverlap"]


def _check_counts_alone(P, counters, want, seed, lo, hi):
    """counts without lists: when only segment-side counters are asked for, the count kernel may take the units as
    k_tail left them (merged list + record, no k_finalize); the same numbers must come out -- of both that path and the
    final lists (GAT_COUNT_FINAL_LISTS)"""
    for sub in (SEGMENT_SIDE, ["nucleotide-overlap"], ["segment-overlap"]):
        got = P.sample_and_count(sub, seed, lo, hi)
        for k, c in enumerate(sub):
            assert np.array_equal(got[k], want[counters.index(c)]), ("counts alone", c, P.last_stats["lists_from_records"])
    P.ctx.options["GAT_COUNT_FINAL_LISTS"] = "1"
    try:
        got = P.sample_and_count(SEGMENT_SIDE, seed, lo, hi)
    finally:
        P.ctx.options.pop("GAT_COUNT_FINAL_LISTS", None)
    for k, c in enumerate(SEGMENT_SIDE):
        assert np.array_equal(got[k], want[counters.index(c)]), ("final lists", c)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_random_problems_vs_oracle(ctx, seed):
    rs = np.random.RandomState(seed)
    flat = _random_problem(rs, n_contigs=int(rs.randint(1, 6)), n_segs=int(rs.randint(20, 600)),
                           n_tracks=int(rs.randint(1, 5)), isochores=bool(seed % 2), dense=(seed % 3 == 0))
    counters = list(_lib.COUNTER_IDS.keys())
    S = 40
    want, wsamples = O.run_samples(flat, counters, 1000 + seed, 1, 5, 5 + S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 1000 + seed, 5, 5 + S)
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), c
    seg, off = P.sample(1000 + seed, 5, 5 + S)
    assert np.array_equal(off, wsamples[1])
    assert np.array_equal(seg, wsamples[0])
    _check_counts_alone(P, counters, want, 1000 + seed, 5, 5 + S)
    P.close()


def test_shard_independence(ctx):
    """any split of the sample range gives the same columns (multi-GPU sharding relies on it)."""
    z = np.load(os.path.join(G, "run_small_isochores.npz"))
    P = _lib.Problem(ctx, _flat(z))
    counters = ["nucleotide-overlap", "nucleotide-density"]
    full = P.sample_and_count(counters, 5, 0, 64)
    a = P.sample_and_count(counters, 5, 0, 23)
    b = P.sample_and_count(counters, 5, 23, 64)
    for k in range(2):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), full[k])
    P.close()


def test_count_lists_vs_oracle(ctx):
    rs = np.random.RandomState(9)
    n_groups, n_tracks, n_lists = 3, 4, 2
    lists, annos = [], []
    for _ in range(n_lists * n_groups):
        lists.append(O.normalize([(int(a), int(a + b)) for a, b in zip(rs.randint(0, 50000, 80), rs.randint(1, 300, 80))]))
    for _ in range(n_tracks * n_groups):
        annos.append(O.normalize([(int(a), int(a + b)) for a, b in zip(rs.randint(0, 50000, 60), rs.randint(1, 900, 60))]))
    off = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)  # noqa: E731
    ws_nseg = [3, 1, 7]
    counters = list(_lib.COUNTER_IDS.keys())
    got = ctx.count_lists(counters, np.concatenate(lists), off(lists), n_lists, np.concatenate(annos), off(annos),
                          n_tracks, ws_nseg, n_groups)
    for k, c in enumerate(counters):
        for t in range(n_tracks):
            for l in range(n_lists):
                vals = [O.counter(c, lists[l * n_groups + g], annos[t * n_groups + g], ws_nseg[g]) for g in range(n_groups)]
                if c == "nucleotide-density":
                    acc = 0.0
                    for v in vals:
                        acc += v
                    assert got[k][t, l] == acc
                else:
                    assert got[k][t, l] == int(sum(vals))


def test_roundtrip_invariants_full_size(ctx):
    """BASELINE config-2 size, properties the reference's own benchmark suite states
    (test/benchmark_gat.py:773-780, :828-837): every sampled list is normalized, lies in the
    workspace, and covers exactly the observed number of workspace bases."""
    cfg = synthetic.config("config2")
    from gat_amd import problem
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], None)
    P = _lib.Problem(ctx, flat)
    S = 64
    seg, off = P.sample(77, 1000, 1000 + S)
    C = flat["n_contigs"]
    for c in range(C):
        u = list(flat["unit_contig"]).index(c)
        us = flat["segs"][flat["seg_off"][u]:flat["seg_off"][u + 1]]
        uw = flat["ws"][flat["ws_off"][u]:flat["ws_off"][u + 1]]
        ltotal = O.total(O.intersect(O.filter(us, uw), uw))
        for i in range(S):
            x = seg[off[i * C + c]:off[i * C + c + 1]]
            assert O.check(x)
            assert O.total(O.intersect(x, uw)) == ltotal
            assert len(O.filter(x, uw)) == len(x)
    counts = P.sample_and_count(["nucleotide-overlap"], 77, 1000, 1000 + S)[0]
    a = flat["annos"]
    for i in range(0, S, 9):
        tot = 0
        for c in range(C):
            x = seg[off[i * C + c]:off[i * C + c + 1]]
            tot += O.overlap_with_segments(x, a[flat["anno_off"][c]:flat["anno_off"][c + 1]])
        assert counts[0, i] == tot
    P.close()


def test_run_api_rows_match_reference(ctx):
    """gat_amd.run() end to end (observed counts, sampled counts, statistics, 24-column rows)
    against the rows the reference's AnnotatorResultExtended printed for the same count matrix."""
    import gat_amd
    z = np.load(os.path.join(G, "run_small_isochores.npz"))
    _, cfg = synthetic.small_genome()

    def coll(tracks):
        c = gat_amd.IntervalCollection()
        for t, per in tracks:
            for contig, a in per.items():
                s = gat_amd.SegmentList(array=a)
                s.isNormalized = 1
                c.add(t, contig, s)
        return c

    segments = coll([("merged", cfg["segments"])])
    annotations = coll(cfg["annotations"])
    workspaces = coll([("ws", cfg["workspace"])])
    workspaces.collapse()
    workspaces.restrict("collapsed")
    isochores = coll(list(cfg["isochores"].items()))
    isochores.intersect(workspaces["collapsed"])
    workspaces.toIsochores(isochores, truncate=True)
    annotations.toIsochores(isochores, truncate=True)
    segments.toIsochores(isochores, truncate=False)
    counters = [gat_amd.COUNTERS[str(c)]() for c in z["counters"]]
    results = gat_amd.run(segments, annotations, workspaces["collapsed"], gat_amd.SamplerAnnotator(bucket_size=0),
                          counters, gat_amd.UnconditionalWorkspace(), num_samples=int(z["num_samples"]),
                          random_seed=int(z["seed"]))
    rows = [str(r) for r in results]
    assert rows == [str(x) for x in z["rows_mode1"]]
    for r in results:
        k = [str(c) for c in z["counters"]].index(r.counter)
        a = [str(t) for t in z["track_names"]].index(r.annotation)
        assert r.observed == z["observed"][k, a]
    # ... and with the reference's own stream (one MT19937 for the whole run): the rows of the UNPATCHED reference
    results0 = gat_amd.run(segments, annotations, workspaces["collapsed"], gat_amd.SamplerAnnotator(bucket_size=0),
                           counters, gat_amd.UnconditionalWorkspace(), num_samples=int(z["num_samples"]),
                           random_seed=int(z["seed"]), reference_stream=True)
    assert [str(r) for r in results0] == [str(x) for x in z["rows_mode0"]]


def _big_problem(rs, n_segs, ws_pieces, n_contigs=2, mean_len=80):
    import collections
    from gat_amd import problem
    contigs = collections.OrderedDict(("k%d" % i, 3000000 + 500000 * i) for i in range(n_contigs))
    segs = synthetic.random_segments(contigs, n_segs, mean_len, int(rs.randint(1 << 30)))
    annos = [("t0", synthetic.random_segments(contigs, 500, 1500, int(rs.randint(1 << 30))))]
    ws = synthetic.workspace_ungapped(contigs, pieces=ws_pieces, gap=600)
    return problem.flatten_arrays(segs, annos, ws, None)


@pytest.mark.parametrize("case", ["many_workspace_segments", "large_units", "large_units_swapped_count", "rows_run_out",
                                  "slab_overflow_retry", "slab_overflow_retry_batches_shrink", "large_units_many_workspace_segments",
                                  "large_units_one_workspace_segment", "mid_workspace_table", "very_large_unit"])
def test_robustness_paths_vs_oracle(ctx, case, monkeypatch):
    """code paths the BASELINE shapes do not reach: workspace lists beyond the register / LDS tables,
    units beyond the register sort, streams that run out of pre-generated rows (redone from the seed),
    and slab overflow (batch redone with doubled capacity).  All must stay bit-exact."""
    import zlib
    rs = np.random.RandomState(zlib.crc32(case.encode()) % 1000)
    if case == "many_workspace_segments":          # k_place: rank table in LDS, two-level workspace table
        flat = _big_problem(rs, 900, 400)
    elif case == "large_units_many_workspace_segments":   # rank table and workspace both beyond the LDS tables
        flat = _big_problem(rs, 6000, 400)
    elif case == "large_units_one_workspace_segment":     # single-segment loop with the rank table in global memory
        flat = _big_problem(rs, 6000, 1)
    elif case == "mid_workspace_table":                   # 65..256 workspace segments: LDS table, beyond k_sampler's registers
        flat = _big_problem(rs, 900, 150)
    elif case in ("large_units", "large_units_swapped_count"):
        flat = _big_problem(rs, 6000, 3)
    elif case == "very_large_unit":                       # 13 500 segments drawn, 11 722 after normalization: one list beyond k_merge_big's
        #                                                   registers (ccap 12 800 > 12 288: its two-pass form), within LDS (asserted below)
        flat = _big_problem(rs, 13500, 1, n_contigs=1, mean_len=30)
    elif case == "rows_run_out":
        monkeypatch.setitem(ctx.options, "GAT_RNG_SLACK", "0.6")
        flat = _big_problem(rs, 700, 5)
    elif case == "slab_overflow_retry_batches_shrink":
        # a scratch budget of about 15 samples: the 24 samples run in batches, and after the overflow the doubled regions
        # make the batch that fits the budget smaller -- the remaining samples must be re-batched, not refused
        monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
        monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "300000")
        flat = _big_problem(rs, 700, 5)
    else:
        monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
        flat = _big_problem(rs, 700, 5)
    counters = ["nucleotide-overlap", "segment-overlap", "annotation-overlap"]
    if case == "large_units_swapped_count":        # overlap counters only: sample lists indexed, tracks streamed
        counters = ["nucleotide-density", "nucleotide-overlap"]
    S = 24
    want, wsamples = O.run_samples(flat, counters, 99, 1, 3, 3 + S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 99, 3, 3 + S)
    st = P.last_stats
    planned = ctx.sampler_report()
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), (case, c)
    seg, off = P.sample(99, 3, 3 + S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    if case == "very_large_unit":
        assert (planned["long_lists"], planned["merge_big"], planned["huge"], planned["big_buckets"]) == (1, 1, 0, 0), planned
        assert planned["classes"][0]["merge_form"] == 0 and planned["classes"][0]["merge_ccap"] > 12288, planned
    if case == "rows_run_out":
        # (a stream that runs out of pre-generated rows goes on from the generator moved up to its position; only SamplerSegments
        #  and long lists behind k_tail_big are still run in full)
        assert st["n_resumed_units"] > 0 and st["n_full_units"] == 0
    if case in ("large_units", "large_units_one_workspace_segment"):
        # long lists: k_merge_big, then k_tail_big carries the units through their placement rounds
        assert st["n_tail_units"] > 0.5 * S * flat["n_units"], st["n_tail_units"]
        ctx.options["GAT_NO_TAIL_BIG"] = "1"
        try:
            other = P.sample_and_count(counters, 99, 3, 3 + S)
            assert P.last_stats["n_tail_units"] == 0
        finally:
            ctx.options.pop("GAT_NO_TAIL_BIG", None)
        for k in range(len(counters)):
            assert np.array_equal(other[k], want[k])
        ctx.options["GAT_NO_RESUME_BIG"] = "1"            # ... and k_sampler, not k_resume_big, finishing them
        try:
            other = P.sample_and_count(counters, 99, 3, 3 + S)
            seg2, off2 = P.sample(99, 3, 3 + S)
        finally:
            ctx.options.pop("GAT_NO_RESUME_BIG", None)
        for k in range(len(counters)):
            assert np.array_equal(other[k], want[k])
        assert np.array_equal(off2, wsamples[1]) and np.array_equal(seg2, wsamples[0])
    if case.startswith("slab_overflow_retry"):
        assert st["n_retried"] > 0
    P.close()


def _long_list_case(ctx, seed):
    """long lists (k_merge_big + k_tail_big + k_sampler's resume) at coverages from sparse to crowded: new segments that
    touch nothing, touch one neighbour (united in place), touch several (handed back), rounds that end in a trim or not"""
    import collections
    from gat_amd import problem
    rs = np.random.RandomState(seed)
    contigs = collections.OrderedDict(("L%d" % i, int(rs.randint(400000, 4000000))) for i in range(int(rs.randint(1, 3))))
    n_segs = int(rs.choice([1300, 2500, 5000]))
    size = sum(contigs.values())
    mean_len = max(2, int(size * float(rs.choice([0.005, 0.03, 0.1, 0.3])) / n_segs))
    segs = synthetic.random_segments(contigs, n_segs, mean_len, int(rs.randint(1 << 30)))
    annos = [("t0", synthetic.random_segments(contigs, 300, 2000, int(rs.randint(1 << 30))))]
    ws = synthetic.workspace_ungapped(contigs, pieces=int(rs.choice([1, 1, 4])), gap=500)
    # (every fifth seed: two isochore classes in blocks of 0.1-0.3 Mb -- long lists whose readers are k_contig, or k_count_merged on the
    #  concatenated lists with k_units_overlap's probes: what k_tail_big's bridges leave empty in a list must not be met as a segment)
    iso = synthetic.isochores_blocks(contigs, nclasses=2, block=int(rs.choice([100000, 300000]))) if seed % 5 == 0 else None
    flat = problem.flatten_arrays(segs, annos, ws, iso, bucket_size=int(rs.choice([0, 1])), nbuckets=100000)
    # odd seeds: the nucleotide counters alone, through the merged index -- the route on which k_resume_big leaves what a
    # trim emptied in the list as [0, 0) instead of compacting it (the config-4 shape's route)
    loose = seed % 2 == 1
    counters = ["nucleotide-overlap", "nucleotide-density"] if loose else ["nucleotide-overlap", "segment-overlap"]
    S = 5
    want, wsamples = O.run_samples(flat, counters, seed, 1, 0, S, want_samples=True)
    if loose:
        ctx.options["GAT_MERGED_MIN_TRACKS"] = "1"
        if seed % 4 == 3:                 # ... with the log inserted into the list (round 3's form) instead of left behind it
            ctx.options["GAT_RESUME_INSERT"] = "1"
    if seed % 8 >= 6:                     # ... and a segment that joins two neighbours ending its lane's round, as before round 6
        ctx.options["GAT_TB_NO_BRIDGE"] = "1"
    if seed % 16 >= 12:                   # ... and every step scanning the lane's log
        ctx.options["GAT_TB_NO_LOG_MAP"] = "1"
    if seed % 16 in (2, 3, 10):           # ... and k_merge_big<., 0>: the list read twice, its buckets sorted thread by thread (what lists
        ctx.options["GAT_MERGE_OLD"] = "1"   #     beyond 12 288 segments still take)
    if seed % 32 == 5:                    # ... and k_sampler launched over every unit, not off k_queue_rest's queue
        ctx.options["GAT_NO_LONG_QUEUE"] = "1"
    try:
        P = _lib.Problem(ctx, flat)
        got = P.sample_and_count(counters, seed, 0, S)
        stats = P.last_stats
        seg, off = P.sample(seed, 0, S)
    finally:
        ctx.options.pop("GAT_MERGED_MIN_TRACKS", None)
        ctx.options.pop("GAT_RESUME_INSERT", None)
        ctx.options.pop("GAT_TB_NO_BRIDGE", None)
        ctx.options.pop("GAT_TB_NO_LOG_MAP", None)
        ctx.options.pop("GAT_MERGE_OLD", None)
        ctx.options.pop("GAT_NO_LONG_QUEUE", None)
    if loose:
        assert _lib.COUNT_KERNELS[stats["count_kernel"]] == "k_count_merged"
    handed = stats["n_tail_units"]
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), (c, n_segs, mean_len)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()
    return handed


def _frag_ws_case(ctx, seed, setenv=None):
    """fragmented workspaces (the reference's own test data: 6 600 - 21 000 workspace segments per contig): units of 300 to
    30 000 workspace segments of mixed lengths -- one-base pieces, pieces longer than everything else together, adjacent pieces,
    pieces shorter than the segments placed (a placed segment then reaches over several) -- through k_place_grid (the cdf grid in
    LDS), k_consolidate / k_tail with the position grid, or (knobs by seed) the trees those replaced"""
    import collections
    from gat_amd import problem
    rs = np.random.RandomState(seed)
    n_contigs = int(rs.randint(1, 4))
    style = int(rs.randint(0, 4))
    contigs = collections.OrderedDict()
    ws = collections.OrderedDict()
    for i in range(n_contigs):
        n = int(rs.choice([300, 700, 2000, 6000, 13000, 30000]) * (0.7 + 0.6 * rs.rand())) if i == 0 else int(rs.randint(2, 2000))
        if style == 0:        # kilobase pieces with kilobase gaps (the mouse workspace's shape)
            lens = 1000 + rs.geometric(1.0 / 6000, size=n)
            gaps = rs.geometric(1.0 / 3000, size=n)
        elif style == 1:      # short pieces, many of them shorter than the segments placed; adjacent pieces
            lens = rs.geometric(1.0 / 40, size=n)
            gaps = rs.geometric(1.0 / 30, size=n) - 1
        elif style == 2:      # a few giants among crumbs
            lens = np.where(rs.rand(n) < 0.01, rs.randint(100000, 3000000, size=n), rs.geometric(1.0 / 8, size=n))
            gaps = rs.geometric(1.0 / 200, size=n)
        else:                 # equal pieces
            lens = np.full(n, int(rs.randint(1, 5000)))
            gaps = np.full(n, int(rs.randint(0, 3000)))
        gaps = np.asarray(gaps, dtype=np.int64)
        lens = np.asarray(lens, dtype=np.int64)
        starts = int(rs.randint(0, 5000)) + np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
        keep = starts + lens < (1 << 31) - 10
        a = np.empty(int(keep.sum()), dtype=synthetic.SEG)
        a["start"], a["end"] = starts[keep], (starts + lens)[keep]
        name = "f%d" % i
        ws[name] = a
        contigs[name] = int(a["end"][-1]) + int(rs.randint(1, 5000))
    total = sum(int((a["end"].astype(np.int64) - a["start"]).sum()) for a in ws.values())
    n_segs = int(rs.choice([40, 150, 400, 900]))
    mean_len = max(1, int(min(total * float(rs.choice([0.002, 0.02, 0.1])) / n_segs, 20000)))
    segs = synthetic.random_segments(contigs, n_segs, mean_len, int(rs.randint(1 << 30)))
    annos = [("t0", synthetic.random_segments(contigs, 200, 1500, int(rs.randint(1 << 30))))]
    flat = problem.flatten_arrays(segs, annos, ws, None, bucket_size=int(rs.choice([0, 1, 1, 1])), nbuckets=100000)
    if flat["n_contigs"] == 0:
        return 0
    knobs = {}
    if seed % 2 == 1:
        knobs["GAT_PLACE_NO_CM"] = "1"                 # the compiler's step behind the grid look-ups
    if seed % 8 == 2:
        knobs["GAT_GRID_CELL_SEGS"] = "16"             # coarse grids: long halving searches
    if seed % 8 == 4:
        knobs["GAT_PLACE_NO_GRID"] = "1"               # the trees in global memory (k_place<., 2>)
    if seed % 8 == 6:
        knobs["GAT_TAIL_NO_LONG_WS"] = "1"             # k_sampler alone behind k_place, as before round 6
    counters = ["nucleotide-overlap", "segment-overlap"]
    S = 70 if seed % 3 == 0 else 5                      # (more than a tile of samples now and then)
    try:
        want, wsamples = O.run_samples(flat, counters, seed, 1, 0, S, want_samples=True)
    except ValueError:                                  # (a segment longer than nbuckets x bucket_size: gat/SegmentList.pyx:1170)
        with pytest.raises(ValueError):
            _lib.Problem(ctx, flat)
        return 0
    for k, v in knobs.items():
        ctx.options[k] = v
    try:
        P = _lib.Problem(ctx, flat)
        got = P.sample_and_count(counters, seed, 0, S)
        st = P.last_stats
        for k, c in enumerate(counters):
            assert np.array_equal(got[k], want[k]), (seed, c, style, n_segs, mean_len, knobs)
        seg, off = P.sample(seed, 0, S)
        assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0]), (seed, style, knobs)
        P.close()
    finally:
        for k in knobs:
            ctx.options.pop(k, None)
    return st["n_tail_units"]


def _units_direct_case(ctx, seed):
    """isochore problems counted from the units' lists (k_count_merged<2, .> + k_units_overlap, no k_contig): isochore blocks from
    one base to tens of kilobases against segments of tens to thousands of bases -- segments that reach over the end of their
    block into a neighbouring unit's segment (fromIsochores' merge(0) unites them: gat/Engine.pyx:2857-2876), both of them
    straddlers, a base under three units' segments (the batch is repeated through k_contig)"""
    import collections
    from gat_amd import problem
    rs = np.random.RandomState(seed)
    block = int(rs.choice([1, 7, 100, 1000, 5000, 30000]))
    hi = 400000 if block >= 100 else 20000                         # (one-base blocks: tens of thousands of workspace pieces)
    contigs = collections.OrderedDict(("u%d" % i, int(rs.randint(hi // 20, hi))) for i in range(int(rs.randint(1, 4))))
    nclasses = int(rs.choice([2, 3, 8]))
    size = sum(contigs.values())
    n_segs = int(rs.choice([60, 300, 1200]))
    mean_len = max(1, int(size * float(rs.choice([0.02, 0.1, 0.3])) / n_segs))
    segs = synthetic.random_segments(contigs, n_segs, mean_len, int(rs.randint(1 << 30)))
    n_tracks = int(rs.choice([1, 4, 9]))
    annos = [("t%d" % i, synthetic.random_segments(contigs, 150, 800, int(rs.randint(1 << 30)))) for i in range(n_tracks)]
    ws = synthetic.workspace_ungapped(contigs, pieces=int(rs.choice([1, 3])), gap=int(rs.choice([0, 50, 700])) + 2)
    iso = synthetic.isochores_blocks(contigs, nclasses=nclasses, block=block)
    flat = problem.flatten_arrays(segs, annos, ws, iso, bucket_size=1, nbuckets=100000)
    if flat["n_contigs"] == 0:
        return 0, 0, 0
    counters = ["nucleotide-overlap", "nucleotide-density"]
    S = 70 if seed % 4 == 0 else 6
    try:
        want, _ = O.run_samples(flat, counters, seed, 1, 0, S)
    except ValueError:
        return 0, 0, 0
    ctx.options["GAT_MERGED_MIN_TRACKS"] = "1"
    try:
        P = _lib.Problem(ctx, flat)
        got = P.sample_and_count(counters, seed, 0, S)
        st = P.last_stats
        assert _lib.COUNT_KERNELS[st["count_kernel"]] == "k_count_merged"
        for k, c in enumerate(counters):
            assert np.array_equal(got[k], want[k]), (seed, c, block, nclasses, n_segs, mean_len)
        # ... and once more through the contig lists (k_contig), which must agree
        ctx.options["GAT_COUNT_VIA_CONTIGS"] = "1"
        try:
            other = P.sample_and_count(counters, seed, 0, S)
            assert P.last_stats["n_straddle_candidates"] == 0
        finally:
            ctx.options.pop("GAT_COUNT_VIA_CONTIGS", None)
        for k in range(len(counters)):
            assert np.array_equal(other[k], want[k])
        P.close()
    finally:
        ctx.options.pop("GAT_MERGED_MIN_TRACKS", None)
    return st["n_straddle_candidates"], st["n_unit_overlaps"], st["n_retried"]


@pytest.mark.parametrize("seed", list(range(800, 840)))
def test_isochore_units_counted_directly_vs_oracle(ctx, seed):
    _units_direct_case(ctx, seed)


def test_isochore_units_counted_directly_takes_overlaps_off(ctx):
    """over a handful of seeds the path must have met what it is there for: overlaps between different units' segments
    taken off the sums, and a batch that had to be repeated through k_contig"""
    cands = ovl = retried = 0
    for seed in range(840, 880):
        c, o, r = _units_direct_case(ctx, seed)
        cands, ovl, retried = cands + c, ovl + o, retried + (1 if r else 0)
    assert cands > 0 and ovl > 0 and retried > 0, (cands, ovl, retried)


def test_isochore_units_counted_directly_candidate_buffer_follows_the_call(ctx):
    """the candidate buffer of the concatenated-lists path is sized for a call's batch: a small call first, a large one behind it
    -- the second must not fall back to the sorted lists for want of room (it makes the buffer anew), and a region that
    overflows anyway has the batch repeated with a larger buffer, not the path given up"""
    import collections
    from gat_amd import problem
    contigs = collections.OrderedDict([("k0", 300000), ("k1", 200000)])
    segs = synthetic.random_segments(contigs, 600, 60, 5)
    annos = [("t%d" % i, synthetic.random_segments(contigs, 200, 700, 50 + i)) for i in range(4)]
    ws = synthetic.workspace_ungapped(contigs, pieces=2, gap=500)
    iso = synthetic.isochores_blocks(contigs, nclasses=4, block=20000)
    flat = problem.flatten_arrays(segs, annos, ws, iso, bucket_size=1, nbuckets=100000)
    counters = ["nucleotide-overlap"]
    P = _lib.Problem(ctx, flat)
    try:
        a = P.sample_and_count(counters, 3, 0, 4)
        assert P.last_stats["n_straddle_candidates"] > 0
        b = P.sample_and_count(counters, 3, 0, 700)
        st = P.last_stats
        assert st["n_straddle_candidates"] > 0 and st["n_unit_overlaps"] > 0, st      # still the concatenated lists
        want, _ = O.run_samples(flat, counters, 3, 1, 0, 700)
        assert np.array_equal(b[0], want[0]) and np.array_equal(a[0], want[0][:, :4])
    finally:
        P.close()
    # regions of one entry: they overflow, the batch is repeated with four times the buffer until it holds -- still this path
    ctx.options["GAT_TEST_SMALL_CAPS"] = "1"
    try:
        P = _lib.Problem(ctx, flat)
        c = P.sample_and_count(counters, 3, 0, 700)
        st = P.last_stats
        assert st["n_retried"] > 0 and st["n_straddle_candidates"] > 0 and np.array_equal(c[0], want[0]), st
        P.close()
    finally:
        ctx.options.pop("GAT_TEST_SMALL_CAPS")


@pytest.mark.parametrize("seed", list(range(700, 732)))
def test_fragmented_workspaces_vs_oracle(ctx, seed):
    _frag_ws_case(ctx, seed)


@pytest.mark.parametrize("sampler", [0, 1])
def test_wide_placement_tiles_vs_oracle(ctx, sampler):
    """k_place_wide (units of thousands of segments on one workspace segment: eight tiles of a unit per workgroup around
    the unit's rank table in LDS) over more than one workgroup, the last one with idle waves and a ragged tile: 600 samples
    = 10 tiles; both sampler kinds; counts and sampled lists against the oracle."""
    import collections
    from gat_amd import problem
    contigs = collections.OrderedDict([("W0", 3000000), ("W1", 1700000)])
    segs = synthetic.random_segments(contigs, 4200, 60, 77)
    annos = [("t0", synthetic.random_segments(contigs, 300, 2000, 78))]
    ws = synthetic.workspace_ungapped(contigs, pieces=1, gap=500)
    flat = problem.flatten_arrays(segs, annos, ws, None, bucket_size=1, nbuckets=100000)
    flat["sampler"] = sampler
    # (SamplerSegments without isochores returns raw placement-order lists; counting on them raises as in the reference)
    counters = [] if sampler else ["nucleotide-overlap", "segment-overlap"]
    S = 600
    want, wsamples = O.run_samples(flat, counters, 5, 1, 0, S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    if counters:
        got = P.sample_and_count(counters, 5, 0, S)
        for k, c in enumerate(counters):
            assert np.array_equal(got[k], want[k]), c
    seg, off = P.sample(5, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()


@pytest.mark.parametrize("seed", list(range(900, 912)) + [4513664, 4521821, 4544116])
def test_long_lists_vs_oracle(ctx, seed):
    """(the three seven-digit seeds: tools/fuzz_long.sh's finds of round 6 -- a unit k_tail_big had bridged and then left with ONE
    placed segment went through k_sampler's one-new-segment shortcut, which took the bridge's empty placeholder for a neighbour
    that touches nothing)"""
    _long_list_case(ctx, seed)


@pytest.mark.parametrize("name", ["config1", "config2_s12", "dense", "density_ungapped", "long_segments", "small_contigs",
                                  "small_isochores", "small_isochores_sampler_segments", "small_isochores_truncated"])
def test_reference_stream_matches_the_unpatched_reference(ctx, name):
    """gat_sample_and_count_serial: ONE MT19937 stream for the whole run, seeded as numpy.random.seed(seed), every
    (sample, unit) in the reference's order -- the count matrices the reference's real gat.run produced WITHOUT the
    per-unit re-seeding (counts_mode0 of the goldens), number for number; and the state carries over calls."""
    z = np.load(os.path.join(G, "run_%s.npz" % name), allow_pickle=True)
    flat = dict((k, z[k]) for k in ("n_units", "segs", "seg_off", "ws", "ws_off", "unit_contig", "n_contigs", "merge_contigs",
                                   "n_tracks", "annos", "anno_off", "cws_nseg", "bucket_size", "nbuckets", "sampler"))
    counters = [str(c) for c in z["counters"]]
    S = int(z["num_samples"])
    want = z["counts_mode0"]
    P = _lib.Problem(ctx, flat)
    state = _lib.mt19937_seed(int(z["seed"]))
    got = P.sample_and_count_serial(counters, state, S)
    for k, c in enumerate(counters):
        assert np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)), (name, c)
    # the oracle's mode 0 agrees (it is what pins the oracle to the reference), and two calls continue each other
    owant, _ = O.run_samples(flat, counters, int(z["seed"]), 0, 0, S)
    state = _lib.mt19937_seed(int(z["seed"]))
    cut = S // 3 + 1
    a = P.sample_and_count_serial(counters, state, cut)
    b = P.sample_and_count_serial(counters, state, S - cut)
    for k in range(len(counters)):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), owant[k]), (name, counters[k])
    P.close()


@pytest.mark.parametrize("seed", list(range(40, 52)))
def test_reference_stream_random_problems_vs_oracle(ctx, seed, monkeypatch):
    """the one-stream mode on random problems (isochores, dense units, several contigs and tracks, long lists, slab
    overflow and its repeat from the batch's stream position) against the oracle's mode 0 -- the mode that pins the oracle
    to the reference -- and a run cut into three calls against the same run in one"""
    rs = np.random.RandomState(seed)
    if seed % 4 == 3:
        monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    if seed % 6 == 5:
        flat = _big_problem(rs, 1500, 3, n_contigs=1)
    else:
        flat = _random_problem(rs, n_contigs=int(rs.randint(1, 5)), n_segs=int(rs.randint(20, 500)),
                               n_tracks=int(rs.randint(1, 4)), isochores=bool(seed % 2), dense=(seed % 3 == 0))
    counters = list(_lib.COUNTER_IDS.keys())
    S = 14
    want, _ = O.run_samples(flat, counters, 900 + seed, 0, 0, S)
    P = _lib.Problem(ctx, flat)
    state = _lib.mt19937_seed(900 + seed)
    got = P.sample_and_count_serial(counters, state, S)
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), c
    state2 = _lib.mt19937_seed(900 + seed)
    parts = [P.sample_and_count_serial(counters, state2, n) for n in (3, 1, S - 4)]
    assert np.array_equal(state, state2)
    for k in range(len(counters)):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), want[k])
    P.close()


def test_contig_lists_longer_than_expected(ctx, monkeypatch):
    """k_contig's LDS is sized for the lists a contig is expected to have, not for every unit at its capacity; a batch in
    which a contig's lists do not fit is repeated with the full size (forced here by shrinking the expectation; the same
    switch shrinks the slab regions, so the slab-overflow repeat runs in front of it)"""
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    rs = np.random.RandomState(4242)
    flat = _random_problem(rs, n_contigs=3, n_segs=500, n_tracks=2, isochores=True, dense=False)
    counters = ["nucleotide-overlap", "segment-overlap", "annotation-overlap"]
    S = 20
    want, wsamples = O.run_samples(flat, counters, 5, 1, 0, S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 5, 0, S)
    assert P.last_stats["n_retried"] > 0
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), c
    seg, off = P.sample(5, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()


def _scan_case(ctx, seed, setenv):
    """one random problem of SIMPLE units (one workspace segment per contig, bucket size 1, fewer than 1 024 working segments:
    what k_place_scan takes): counts of all six counters and the sampled lists against the oracle.  Workspaces from a few
    thousand bases -- where every tenth row falls into the band in which the offset draw's acceptance depends on the length,
    and the scan has to be repeated -- to just below a power of two; odd seeds start every chunk from "no offset draw
    accepted" (GAT_PLACE_SCAN_SEQ: the fixed-point loop runs dozens of times per chunk), every third seed keeps the
    lane-per-stream kernels (GAT_PLACE_SCAN_TILES=0) as the cross-check of the cross-check."""
    import collections
    from gat_amd import problem
    rs = np.random.RandomState(seed)
    if seed % 2 == 1:
        setenv("GAT_PLACE_SCAN_SEQ", "1")
    setenv("GAT_PLACE_SCAN_TILES", "0" if seed % 3 == 0 else "100000")
    n_contigs = int(rs.randint(1, 5))
    sizes = [3000, 5000, 40000, (1 << 16) - 3, (1 << 16) + 700, (1 << 20) - 50, 3000000, 150000000]
    contigs = collections.OrderedDict(("g%d" % i, int(rs.choice(sizes)) + int(rs.randint(0, 40))) for i in range(n_contigs))
    mean_len = int(rs.choice([15, 60, 300]))
    total = sum(contigs.values())
    # (at most a tenth of the smallest workspace covered, a unit below 1 024 segments)
    n_segs = int(max(6, min(rs.choice([40, 300, 1500, 3000]), min(contigs.values()) * n_contigs // (10 * mean_len), 900 * n_contigs)))
    segs = synthetic.random_segments(contigs, n_segs, mean_len, int(rs.randint(1 << 30)))
    annos = [("t%d" % t, synthetic.random_segments(contigs, int(rs.randint(5, 300)), int(rs.randint(20, 2000)),
                                                   int(rs.randint(1 << 30)))) for t in range(int(rs.randint(1, 3)))]
    ws = synthetic.workspace_contigs(contigs)
    flat = problem.flatten_arrays(segs, annos, ws, None, bucket_size=1, nbuckets=100000)
    counters = list(_lib.COUNTER_IDS.keys())
    S = int(rs.choice([5, 70, 130]))                         # (a ragged last tile; more than one sample block)
    first = int(rs.randint(0, 1000))
    want, wsamples = O.run_samples(flat, counters, 9000 + seed, 1, first, first + S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(counters, 9000 + seed, first, first + S)
        for k, c in enumerate(counters):
            assert np.array_equal(got[k], want[k]), (c, n_segs, dict(contigs))
        seg, off = P.sample(9000 + seed, first, first + S)
        assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    finally:
        P.close()
    return total


@pytest.mark.parametrize("seed", list(range(400, 436)))
def test_place_scan_vs_oracle(ctx, seed, monkeypatch):
    """k_place_scan (one stream walked by the 64 lanes of a wave, the states as a prefix scan) on random problems of simple
    units: bit-exact with the oracle, with the scan's fixed-point loop forced on odd seeds"""
    _scan_case(ctx, seed, lambda k, v: monkeypatch.setitem(ctx.options, k, v))


@pytest.mark.parametrize("seed", list(range(100, 164)) + [1508540, 1549729, 1552333])     # (seven digits: as in test_long_lists_vs_oracle)
def test_fuzz_shapes_vs_oracle(ctx, seed, monkeypatch):
    """random combinations of the knobs that select code paths -- segments per unit (register / bucket / counting
    sorts), workspace pieces (registers / LDS table / search trees), bucket size (with and without the bucket draw),
    isochores, sampler kind -- against the oracle: counts for all six counters and the sampled lists."""
    import collections
    from gat_amd import problem
    if seed % 6 == 0:
        monkeypatch.setitem(ctx.options, "GAT_TEST_HUGE", "1")          # ... and the list-in-global-memory variants
    if seed % 2 == 1:
        # (a call of a few samples of simple units takes k_place_wide by itself: every other seed keeps the lean kernels)
        monkeypatch.setitem(ctx.options, "GAT_PLACE_NO_WIDE", "1")
    if seed % 4 >= 2:
        # (k_place's written-out steps take every unit they can: half the seeds keep the compiler's form of the same steps,
        #  which is what units with a bucket draw, SamplerSegments and offset masks that depend on the length still run)
        monkeypatch.setitem(ctx.options, "GAT_PLACE_NO_CM", "1")
    rs = np.random.RandomState(seed)
    n_contigs = int(rs.randint(1, 4))
    contigs = collections.OrderedDict(("f%d" % i, int(rs.randint(200000, 3000000))) for i in range(n_contigs))
    n_segs = int(rs.choice([30, 150, 700, 2500]))
    mean_len = int(rs.choice([20, 80, 400]))
    segs = synthetic.random_segments(contigs, n_segs, mean_len, int(rs.randint(1 << 30)))
    annos = [("t%d" % t, synthetic.random_segments(contigs, int(rs.randint(20, 600)), int(rs.randint(50, 3000)),
                                                   int(rs.randint(1 << 30)))) for t in range(int(rs.randint(1, 4)))]
    pieces = int(rs.choice([1, 3, 40, 90, 300]))
    spacing = (min(contigs.values()) - 20000) // pieces
    ws = synthetic.workspace_ungapped(contigs, pieces=pieces, gap=min(int(rs.choice([50, 600])), max(2, spacing // 3)))
    iso = synthetic.isochores_blocks(contigs, nclasses=int(rs.randint(2, 4)), block=int(rs.randint(20000, 200000))) \
        if rs.randint(0, 3) == 0 else None
    bucket_size = int(rs.choice([0, 1, 7]))
    nbuckets = 100000 if bucket_size != 1 else 20000
    flat = problem.flatten_arrays(segs, annos, ws, iso, bucket_size=bucket_size, nbuckets=nbuckets)
    # (SamplerSegments output is only countable after fromIsochores merged it: the counters assert normalized lists)
    flat["sampler"] = int(rs.randint(0, 3) == 0 and iso is not None)
    counters = list(_lib.COUNTER_IDS.keys())
    S = 12
    try:
        want, wsamples = O.run_samples(flat, counters, 7000 + seed, 1, 2, 2 + S, want_samples=True)
    except ValueError:                                   # a segment longer than nbuckets * bucket_size
        with pytest.raises(ValueError):
            _lib.Problem(ctx, flat)
        return
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 7000 + seed, 2, 2 + S)
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), (c, n_segs, pieces, bucket_size, iso is not None, flat["sampler"])
    seg, off = P.sample(7000 + seed, 2, 2 + S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    if not flat["sampler"]:
        _check_counts_alone(P, counters, want, 7000 + seed, 2, 2 + S)
    P.close()


@pytest.mark.parametrize("seed", [2, 3])
def test_lists_in_global_memory_vs_oracle(ctx, seed, monkeypatch):
    """the HUGE kernel variants (lists worked on in the slab instead of LDS) forced onto ordinary problems,
    with and without isochores: same counts and sampled lists as the oracle."""
    monkeypatch.setitem(ctx.options, "GAT_TEST_HUGE", "1")
    rs = np.random.RandomState(seed)
    flat = _random_problem(rs, n_contigs=3, n_segs=int(rs.randint(200, 700)), n_tracks=2, isochores=bool(seed % 2))
    counters = ["nucleotide-overlap", "segment-overlap"]
    S = 24
    want, wsamples = O.run_samples(flat, counters, 500 + seed, 1, 0, S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 500 + seed, 0, S)
    for k in range(len(counters)):
        assert np.array_equal(got[k], want[k])
    seg, off = P.sample(500 + seed, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()


def test_unit_beyond_lds_vs_oracle(ctx):
    """one unit with about 45 000 segments (LDS holds about 15 000): the list stays in global memory; the reference has
    no size limit, so neither may the drop-in."""
    rs = np.random.RandomState(11)
    flat = _big_problem(rs, 60000, 2, n_contigs=1, mean_len=20)
    counters = ["nucleotide-overlap"]
    S = 3
    want, wsamples = O.run_samples(flat, counters, 31, 1, 0, S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 31, 0, S)
    assert np.array_equal(got[0], want[0])
    seg, off = P.sample(31, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()


def test_cli_table_matches_reference(ctx, tmp_path):
    """scripts/gat-run.py end to end against the table the reference's gat-run.py printed for the same
    BED files and seed (per-unit stream contract patched into the reference, tests/golden/make_goldens.py)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gat_run_amd", os.path.join(root, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cli = os.path.join(G, "cli")
    with open(os.path.join(cli, "cases.json")) as f:
        cases = json.load(f)
    for name, extra in cases.items():
        extra = [x if not x.startswith("--isochores=") else "--isochores=%s" % os.path.join(cli, "isochores.bed") for x in extra]
        out = str(tmp_path / ("%s.tsv" % name))
        argv = ["gat-run.py", "--segments=%s" % os.path.join(cli, "segments.bed"),
                "--annotations=%s" % os.path.join(cli, "annotations.bed"),
                "--workspace=%s" % os.path.join(cli, "workspace.bed"), "--stdout=%s" % out,
                "--log=%s" % str(tmp_path / "log")] + extra
        assert mod.main(argv) == 0
        got = [l for l in open(out) if not l.startswith("#")]
        want = [l for l in open(os.path.join(cli, "expected_%s.tsv" % name)) if not l.startswith("#")]
        assert got == want, name


def test_cli_reference_stream_matches_the_unpatched_reference(ctx, tmp_path):
    """gat-run.py --reference-stream: the tables the reference's own gat-run.py prints WITHOUT any patch (one numpy stream
    seeded with --random-seed for the whole run: tests/golden/make_goldens.py g5u), byte for byte -- two segment tracks
    and isochores (the stream carries over tracks and units), the density counter with truncation"""
    cli = os.path.join(G, "cli")
    cases = json.load(open(os.path.join(cli, "cases_reference_stream.json")))
    for name, extra in cases.items():
        extra = [x.replace("--isochores=", "--isochores=%s%s" % (cli, os.sep)) for x in extra]
        got = _run_cli(tmp_path, name, ["--segments=%s" % os.path.join(cli, "segments.bed"),
                                        "--annotations=%s" % os.path.join(cli, "annotations.bed"),
                                        "--workspace=%s" % os.path.join(cli, "workspace.bed"), "--reference-stream"] + extra)
        want = [l for l in open(os.path.join(cli, "expected_%s.tsv" % name)) if not l.startswith("#")]
        assert got == want, name


def _run_cli(tmp_path, name, args):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gat_run_amd", os.path.join(root, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / ("%s.tsv" % name))
    assert mod.main(["gat-run.py", "--stdout=%s" % out, "--log=%s" % str(tmp_path / "log")] + args) == 0
    return [l for l in open(out) if not l.startswith("#")]


def test_reference_dataset_bit_exact(ctx, tmp_path):
    """the reference's own integration-test data (test/data/*.bed.gz: mouse ChIP-seq peaks, 279 844 workspace
    segments, 4 segment tracks x 7 annotation tracks): table == what the reference's gat-run.py prints under
    the per-unit stream contract (tests/golden/refdata/expected_mode1_s60.tsv)."""
    d = os.path.join(G, "refdata")
    got = _run_cli(tmp_path, "refdata", ["--segments=%s" % os.path.join(d, "segments_single.bed.gz"),
                                         "--annotations=%s" % os.path.join(d, "annotations.bed.gz"),
                                         "--workspace=%s" % os.path.join(d, "workspace.bed.gz"),
                                         "--num-samples=60", "--random-seed=9", "--with-segment-tracks", "--order=track"])
    want = [l for l in open(os.path.join(d, "expected_mode1_s60.tsv")) if not l.startswith("#")]
    assert got == want


def test_reference_dataset_check_run(ctx, tmp_path):
    """test/check_run.py of the reference, re-expressed: 1000 samples on the same data; `observed` must equal the
    reference's 2013 output (test/data/output_single.tsv) exactly (:109-112), expected / fold / pvalue within its
    tolerances of 10 % max and 5 % mean difference (:33-34, :87-106)."""
    d = os.path.join(G, "refdata")
    got = _run_cli(tmp_path, "check_run", ["--segments=%s" % os.path.join(d, "segments_single.bed.gz"),
                                           "--annotations=%s" % os.path.join(d, "annotations.bed.gz"),
                                           "--workspace=%s" % os.path.join(d, "workspace.bed.gz"),
                                           "--num-samples=1000", "--random-seed=1", "--with-segment-tracks"])

    def table(lines):
        hdr = lines[0].rstrip("\n").split("\t")
        return dict(((f[0], f[1]), dict(zip(hdr, f))) for f in (l.rstrip("\n").split("\t") for l in lines[1:]))

    ref = table([l for l in open(os.path.join(d, "output_single.tsv")) if not l.startswith("#")])
    mine = table(got)
    assert set(ref.keys()) == set(mine.keys()) and len(ref) == 28
    for col in ("observed", "track_nsegments", "track_size", "annotation_nsegments", "annotation_size",
                "overlap_nsegments", "overlap_size"):
        for k in ref:
            assert mine[k][col] == ref[k][col], (k, col)
    for col in ("expected", "fold", "pvalue"):
        diffs = []
        for k in ref:
            a, b = float(mine[k][col]), float(ref[k][col])
            diffs.append(0.0 if a == b else 100.0 * abs(a - b) / max(abs(a), abs(b)))
        assert max(diffs) < 10.0 and sum(diffs) / len(diffs) < 5.0, (col, max(diffs))


def test_sampler_segments_vs_oracle(ctx, monkeypatch):
    """SamplerSegments (gat/Engine.pyx:653): raw placement-order lists without isochores, merged lists and all
    counters with isochores; counters on un-merged lists raise like the reference's asserts; row exhaustion and
    degenerate units take the wave-per-unit fallback."""
    rs = np.random.RandomState(21)
    for iso in (False, True):
        flat = _random_problem(rs, n_contigs=3, n_segs=250, n_tracks=2, isochores=iso)
        flat["sampler"] = 1
        want_c, wsamples = (None, None)
        counters = list(_lib.COUNTER_IDS.keys()) if iso else []
        want_c, wsamples = O.run_samples(flat, counters, 77, 1, 2, 34, want_samples=True)
        P = _lib.Problem(ctx, flat)
        seg, off = P.sample(77, 2, 34)
        assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
        if iso:
            got = P.sample_and_count(counters, 77, 2, 34)
            for k, c in enumerate(counters):
                assert np.array_equal(got[k], want_c[k]), c
        else:
            with pytest.raises(AssertionError):
                P.sample_and_count(["nucleotide-overlap"], 77, 2, 34)
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_RNG_SLACK", "0.5")
    flat = _random_problem(rs, n_contigs=2, n_segs=300, n_tracks=1, isochores=False)
    flat["sampler"] = 1
    _, wsamples = O.run_samples(flat, [], 5, 1, 0, 20, want_samples=True)
    P = _lib.Problem(ctx, flat)
    seg, off = P.sample(5, 0, 20)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    assert P.last_stats["n_full_units"] > 0
    P.close()


def test_error_behaviour_and_edge_cases(ctx):
    """errors mirror the reference: non-normalized input -> AssertionError (gat/Engine.pyx:535-536),
    segment longer than nbuckets*bucket_size -> ValueError (gat/SegmentList.pyx:1170), coordinates >= 2^31 ->
    ValueError; empty units / empty annotation lists / zero samples are handled."""
    w = [(0, 100000)]
    with pytest.raises(AssertionError):
        _lib.Problem(ctx, _single_unit_flat([(10, 50), (40, 90)], w, 0, 100000))          # overlapping segments
    with pytest.raises(AssertionError):
        _lib.Problem(ctx, _single_unit_flat([(10, 50)], [(500, 900), (0, 100)], 0, 100000))  # unsorted workspace
    with pytest.raises(ValueError):
        _lib.Problem(ctx, _single_unit_flat([(0, 500), (1000, 201000)], [(0, 1000000)], 1, 100000))
    with pytest.raises(ValueError):
        _lib.Problem(ctx, _single_unit_flat([(10, 50)], [(0, 2200000000)], 0, 100000))
    # a unit whose segments all lie outside its workspace gives an empty list and consumes nothing
    s = O.segs([(5000, 5100), (7000, 7050)])
    flat = dict(n_units=2, segs=np.concatenate([s, O.segs([(10, 60), (200, 260)])]), seg_off=[0, 2, 4],
                ws=O.segs([(0, 1000), (0, 1000)]), ws_off=[0, 1, 2], unit_contig=[0, 1], n_contigs=2, merge_contigs=0,
                n_tracks=2, annos=O.segs([(0, 400), (100, 300)]), anno_off=[0, 0, 1, 2, 2], cws_nseg=[1, 1],
                bucket_size=0, nbuckets=100000)
    P = _lib.Problem(ctx, flat)
    counters = list(_lib.COUNTER_IDS.keys())
    got = P.sample_and_count(counters, 3, 0, 9)
    want, wsamples = O.run_samples(flat, counters, 3, 1, 0, 9, want_samples=True)
    for k in range(len(counters)):
        assert np.array_equal(got[k], want[k])
    seg, off = P.sample(3, 0, 9)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    assert all(off[2 * i + 1] == off[2 * i] for i in range(9))            # contig 0 always empty
    for g in P.sample_and_count(counters, 3, 4, 4):                        # zero samples
        assert g.shape == (2, 0)
    P.close()
    # counters on empty lists
    r = ctx.count_lists(counters, O.segs([]), [0, 0], 1, O.segs([(0, 10)]), [0, 1], 1, [1], 1)
    assert all(x[0, 0] == 0 for x in r)
    r = ctx.count_lists(counters, O.segs([(0, 10)]), [0, 1], 1, O.segs([]), [0, 0], 1, [1], 1)
    assert all(x[0, 0] == 0 for x in r)


def test_host_classes_on_device(ctx):
    """SegmentList.overlapWithSegments / intersectionWithSegments and Counter.__call__ run on the device and agree
    with the reference-generated pair goldens (tests/golden/algebra.json)."""
    import gat_amd
    with open(os.path.join(G, "algebra.json")) as f:
        cases = [c for c in json.load(f) if c["op"] == "pair"][:40]
    for c in cases:
        a = gat_amd.SegmentList(iter=c["a"], normalize=True)
        b = gat_amd.SegmentList(iter=c["b"], normalize=True)
        assert a.overlapWithSegments(b) == c["overlap"]
        assert a.intersectionWithSegments(b) == c["isect_base"]
        assert a.intersectionWithSegments(b, mode="midpoint") == c["isect_mid"]
        assert gat_amd.CounterAnnotationOverlap()(a, b) == c["isect_base_rev"]
        assert gat_amd.CounterNucleotideOverlap()(a, b) == c["overlap"]
    s = gat_amd.SegmentList(iter=[(x, x + 100) for x in range(0, 10000, 1000)], normalize=True)
    w = gat_amd.SegmentList(iter=[(0, 10000)], normalize=True)
    r = gat_amd.SamplerAnnotator(bucket_size=1, nbuckets=100000).sample(s, w, seed=5)
    rng = O.RandomState(5)
    want, _ = O.sampler_annotator(rng, s.asList(), w.asList(), 1, 100000)
    assert r.asList() == O.aslist(want)


def test_knobs_are_options_of_a_context_not_the_environment(ctx):
    """gat_ctx_set_option: a knob's value is the context's own, else the process's environment AS THE LIBRARY FIRST SAW IT --
    nothing reads the environment on a call's path, and a second context does not see what the first one set"""
    key = "GAT_COUNT_FINAL_LISTS"
    assert ctx.options.get(key) is None
    os.environ[key] = "1"                                   # (behind the snapshot: not seen)
    try:
        assert ctx.options.get(key) is None
    finally:
        del os.environ[key]
    other = _lib.Context(0)
    try:
        ctx.options[key] = "1"
        assert ctx.options.get(key) == "1" and other.options.get(key) is None
        ctx.options[key] = ""                               # "not set", whatever the environment says
        assert ctx.options.get(key) is None
        del ctx.options[key]
        assert key not in ctx.options and ctx.options.get(key) is None
        with pytest.raises((ValueError, _lib.GatError)):     # (GAT_ERR_ARG)
            other.options["NOT_A_GAT_KEY"] = "1"
    finally:
        other.close()
    # ... and it acts: the same problem with and without the final lists (a knob read at the call)
    _, cfg = synthetic.small_genome()
    from gat_amd import problem
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], None)
    P = _lib.Problem(ctx, flat)
    try:
        a = P.sample_and_count(["nucleotide-overlap"], 5, 0, 16)
        rec = P.last_stats["lists_from_records"]
        ctx.options[key] = "1"
        try:
            b = P.sample_and_count(["nucleotide-overlap"], 5, 0, 16)
            assert P.last_stats["lists_from_records"] == 0 and rec > 0
        finally:
            ctx.options.pop(key)
        assert np.array_equal(a[0], b[0])
    finally:
        P.close()


def test_a_knob_acts_on_what_starts_after_it_was_set(ctx):
    """The knobs are read into one snapshot per problem, per annotation object and per call (gat_knobs.h): a set_option acts on
    what is created or called after it.  The annotation tables -- built by a thread of the library while the caller goes on --
    are those of the knobs as they were when gat_annotations_create was called, whatever the caller sets meanwhile; a problem
    keeps the path it was created for; a knob of the call acts on the next call."""
    from gat_amd import problem
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"][:2], cfg["workspace"], None)
    counters, seed, S = ["nucleotide-overlap"], 5, 16
    want, _ = O.run_samples(flat, counters, seed, 1, 0, S)

    def count(P):
        got = P.sample_and_count(counters, seed, 0, S)
        assert np.array_equal(got[0], want[0])
        return P.last_stats

    # two tracks take the per-track kernel; "from one track up" set for the length of the create call alone: the merged index
    ctx.options["GAT_MERGED_MIN_TRACKS"] = "1"
    try:
        A = _lib.Annotations(ctx, flat, asynchronous=True)
    finally:
        del ctx.options["GAT_MERGED_MIN_TRACKS"]              # (back to 4 while the tables are being built)
    P = _lib.Problem(ctx, flat, annotations=A)
    try:
        A.wait()
        assert _lib.COUNT_KERNELS[count(P)["count_kernel"]] == "k_count_merged"
    finally:
        P.close()
        A.close()
    # ... and set only after the create call: no index
    A = _lib.Annotations(ctx, flat, asynchronous=True)
    ctx.options["GAT_MERGED_MIN_TRACKS"] = "1"
    try:
        P = _lib.Problem(ctx, flat, annotations=A)
        try:
            A.wait()
            assert _lib.COUNT_KERNELS[count(P)["count_kernel"]] == "k_count_seg"
        finally:
            P.close()
            A.close()
    finally:
        del ctx.options["GAT_MERGED_MIN_TRACKS"]
    # a knob of the creation: a problem made under GAT_NO_SPLIT keeps k_sampler behind k_place (k_tail finishes no unit) when the
    # option is gone, one made without it keeps the split path when the option comes
    ctx.options["GAT_NO_SPLIT"] = "1"
    try:
        P_plain = _lib.Problem(ctx, flat)
    finally:
        del ctx.options["GAT_NO_SPLIT"]
    P_split = _lib.Problem(ctx, flat)
    try:
        st = count(P_plain)
        assert st["n_tail_units"] == 0 and st["lists_from_records"] == 0
        ctx.options["GAT_NO_SPLIT"] = "1"
        try:
            st = count(P_split)
        finally:
            del ctx.options["GAT_NO_SPLIT"]
        assert st["n_tail_units"] > 0 and st["lists_from_records"] > 0
        # a knob of the call: set after the creation, it acts on the next call
        ctx.options["GAT_COUNT_FINAL_LISTS"] = "1"
        try:
            assert count(P_split)["lists_from_records"] == 0
        finally:
            del ctx.options["GAT_COUNT_FINAL_LISTS"]
        assert count(P_split)["lists_from_records"] > 0
    finally:
        P_plain.close()
        P_split.close()


def test_wave_only_sampler_mode(ctx, monkeypatch):
    """GAT_SAMPLER_MODE=wave: the stand-alone wave-per-unit sampler (own MT19937 in LDS, no k_rng / k_place),
    which is also the fallback path of the default pipeline, gives the same bits."""
    monkeypatch.setitem(ctx.options, "GAT_SAMPLER_MODE", "wave")
    z = np.load(os.path.join(G, "run_small_isochores.npz"))
    counters = [str(c) for c in z["counters"]]
    P = _lib.Problem(ctx, _flat(z))
    counts = P.sample_and_count(counters, int(z["seed"]), 0, int(z["num_samples"]))
    for k, c in enumerate(counters):
        want = z["counts_mode1"][k]
        assert np.array_equal(counts[k] if c == "nucleotide-density" else counts[k].astype(np.float64), want), c
    assert P.last_stats["n_full_units"] > 0
    P.close()


def _torchrun(nproc, script_args, env, root, timeout):
    """`python -m torch.distributed.run --nproc-per-node N bench.py ...` the way the driver launches it, on a port found free
    -- and once more on another one should somebody have taken it in between (EADDRINUSE)"""
    import socket
    import subprocess
    import sys
    for attempt in range(3):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(port)] + script_args
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
        if r.returncode == 0 or "EADDRINUSE" not in r.stderr:
            break
    return r


def _bench_outputs(r, details):
    """(the ONE stdout line of a bench.py run -- small, the last thing printed --, its details file)"""
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len([l for l in lines if l.startswith("{")]) == 1 and lines[-1].startswith("{")
    assert len(lines[-1]) < 4096, len(lines[-1])
    return json.loads(lines[-1]), json.load(open(details))


def test_bench_default_line_is_small_and_honest(tmp_path):
    """one rank, the real run: the line the driver parses is below 4 KB, carries roofline + cpu_baseline, and its
    value / ms_per_step are the K steps timed right behind the W warm-up steps (value = samples x K / that time)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    details = str(tmp_path / "details.json")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "4", "--warmup", "2", "--extra", "config3", "--extra-steps", "2",
           "--no-strong", "--no-api", "--sustain-seconds", "0.2", "--cpu-seconds", "2", "--details", details]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line, full = _bench_outputs(r, details)
    assert line["steps"] == 4 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["vs_baseline"] is None
    assert line["value"] == pytest.approx(10000 * 1e3 / line["ms_per_step"], rel=1e-3)
    assert line["value"] == pytest.approx(full["value"], rel=1e-5)
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    assert line["roofline"]["frac"] == pytest.approx(line["roofline"]["achieved"] / line["roofline"]["peak"], rel=1e-3)
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1
    assert full["configs"]["config3"]["cpu_baseline"]["value"] > 0       # the north_star target shape has its own
    assert full["sustained"]["seconds"] >= 0.2 and "kernels" in full and "sampler" in full


def test_bench_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    """a run without --full: the K steps and nothing else (no cpu_baseline, no extra shapes, no sustained loop, no per-kernel
    steps), value / ms_per_step of exactly those steps, and --dump-outputs writes the last timed step's count matrix, equal to
    the oracle's columns for its sample ids"""
    import subprocess
    import sys
    from gat_amd import problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    details, dump = str(tmp_path / "details.json"), str(tmp_path / "outputs")
    S, K, W = 256, 3, 2
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--samples", str(S),
           "--dump-outputs", dump, "--details", details]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line, out = _bench_outputs(r, details)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in line, k
    assert line["steps"] == K and line["warmup"] == W and line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(S * 1e3 / line["ms_per_step"], rel=1e-3)
    assert line["value_source"].startswith("the %d timed steps" % K)
    for k in ("cpu_baseline", "configs", "strong_scaling", "api", "sustained", "kernels", "sampler"):
        assert k not in out, k
    assert os.listdir(dump) == ["counts.npy"]
    got = np.load(os.path.join(dump, "counts.npy"))
    assert got.dtype == np.float64 and got.shape == (1, 1, S)
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"])
    first = (W + K - 1) * S                               # the last timed step's sample ids
    want, _ = O.run_samples(flat, [cfg["counter"]], 12345, 1, first, first + S)
    assert np.array_equal(got[0], want[0].astype(np.float64))


def test_bench_two_ranks_on_one_gpu(tmp_path):
    """bench.py's N > 1 path (rank-disjoint sample ranges, all-gather of the count matrix, max-over-ranks timing,
    one JSON line from rank 0) with two ranks sharing this box's GPU: GAT_BENCH_SHARE_GPU=1 swaps RCCL, which
    refuses two ranks on one device, for gloo; everything else is the code the multi-GPU launch runs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GAT_BENCH_SHARE_GPU="1")
    r = _torchrun(2, [os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "2",
                      "--warmup", "1", "--samples", "2000", "--extra", "", "--no-strong", "--sustain-seconds", "0.2",
                      "--details", str(tmp_path / "d.json")], env, root, 600)
    assert r.returncode == 0, r.stderr[-2000:]
    line, out = _bench_outputs(r, str(tmp_path / "d.json"))
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert line["allgather"]["bytes_per_rank"] == 2000 * 8 and out["allgather"]["bytes_per_rank"] == 2000 * 8
    assert "cpu_baseline" not in line and "cpu_baseline" not in out and "api" not in out # reported at N = 1 only
    assert out["sustained"]["seconds"] >= 0.2 and out["sustained"]["min"] <= out["sustained_value"] <= out["sustained"]["max"]
    assert line["sustained_value"] == pytest.approx(out["sustained_value"], rel=1e-5)


def test_bench_leaves_a_line_when_a_rank_fails(tmp_path):
    """a rank that dies behind the roll call takes the job down -- non-zero exit, no hang -- and rank 0 still leaves ONE JSON
    line: value null, the error, and who was there (world size, backend, the ranks' devices, the collective's own count)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GAT_BENCH_SHARE_GPU="1", GAT_BENCH_FAIL_RANK="1", GAT_BENCH_DIST_TIMEOUT="60")
    r = _torchrun(2, [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--samples", "500", "--extra", "",
                      "--no-strong", "--sustain-seconds", "0", "--details", str(tmp_path / "df.json")], env, root, 300)
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(lines[0])
    assert line["value"] is None and line["error"] and line["n_gpus"] == 2
    d = line["distributed"]
    assert d["world_size"] == 2 and d["ranks_in_collective"] == 2 and len(d["devices"]) == 2 and d["backend"] == "gloo"


def test_bench_eight_ranks_on_one_gpu(tmp_path):
    """the launch the driver's scaling run makes -- eight ranks under torch.distributed.run -- on this box's one GPU (gloo
    instead of RCCL): every rank its own sample range, the gathered matrix of the last step against the oracle's columns"""
    from gat_amd import problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GAT_BENCH_SHARE_GPU="1")
    dump = str(tmp_path / "counts8.npz")
    r = _torchrun(8, [os.path.join(root, "bench.py"), "--full", "--gpus", "8", "--steps", "2",
                      "--warmup", "1", "--samples", "64", "--extra", "", "--sustain-seconds", "0", "--dump-counts", dump,
                      "--details", str(tmp_path / "d8.json")], env, root, 900)
    assert r.returncode == 0, r.stderr[-2000:]
    line, out = _bench_outputs(r, str(tmp_path / "d8.json"))
    assert line["n_gpus"] == 8 and line["distributed"]["world_size"] == 8 and line["value"] > 0
    assert line["distributed"]["ranks_in_collective"] == 8
    assert line["allgather"]["avg_ms"] > 0
    # the metric's own job cut over the eight ranks: measured (every rank its 1 250 samples, the gather, the read-back)
    st = out["strong_scaling"]
    assert st["measured_on"].startswith("8 GPU") and st["config2"]["n8"]["samples_per_gpu"] == 1250
    assert line["strong_scaling"]["config2"]["n8"] > 0 and line["strong_scaling"]["config3"]["n8"] > 0
    assert len(out["distributed"]["devices"]) == 8
    z = np.load(dump)
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"])
    first, S = int(z["first_sample"]), int(z["samples_per_rank"])
    want, _ = O.run_samples(flat, ["nucleotide-overlap"], int(z["seed"]), 1, first, first + 8 * S)
    for rk in range(8):
        assert np.array_equal(z["counts"][rk], want[0][:, rk * S:(rk + 1) * S]), rk


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher in the environment starts its two ranks itself (a child
    torch.distributed.run, before the parent touches a GPU) and relays their one JSON line; one extra shape rides along."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict((k, v) for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"))
    env["GAT_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--samples",
           "1000", "--extra", "config1", "--extra-steps", "1", "--sustain-seconds", "0", "--details", str(tmp_path / "d2.json")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line, out = _bench_outputs(r, str(tmp_path / "d2.json"))
    assert line["n_gpus"] == 2 and line["distributed"]["world_size"] == 2 and line["value"] > 0
    assert out["n_gpus"] == 2 and out["distributed"]["world_size"] == 2 and out["value"] > 0
    assert out["configs"]["config1"]["value"] > 0 and out["configs"]["config1"]["n_gpus"] == 2
    # the metric's own job (10 000 samples in all) cut over the two ranks
    st = out["strong_scaling"]
    assert st["samples_total"] == 10000 and st["config2"]["n2"]["samples_per_gpu"] == 5000 and st["config3"]["n2"]["value"] > 0


def test_cli_overlap_stats_match_reference(ctx, tmp_path):
    """--output-stats=overlap (gat/IO.py:283-289, gat/Engine.pyx:3152-3165; the overlaps are counted on the device)
    against the file the reference wrote for the same inputs."""
    import gat_amd as gat
    from gat_amd import IO
    cli = os.path.join(G, "cli")
    opts, _ = gat.buildParser().parse_args(["--segments=%s" % os.path.join(cli, "segments.bed"),
                                            "--annotations=%s" % os.path.join(cli, "annotations.bed"),
                                            "--workspace=%s" % os.path.join(cli, "workspace.bed"),
                                            "--output-stats=overlap", "-P", str(tmp_path / "%s")])
    segments, annotations, workspaces, isochores = IO.buildSegments(opts)
    IO.applyIsochores(segments, annotations, workspaces, opts, isochores)
    assert open(str(tmp_path / "overlap_merged")).read() == \
        open(os.path.join(cli, "aux", "stats", "overlap_merged_no_isochores")).read()


def test_cli_pattern_outputs_match_reference(ctx, tmp_path):
    """--output-tables-pattern (one table per counter), --output-counts-pattern (the count matrix) and
    --output-samples-pattern (the sampled lists per segment track, at isochore level) byte for byte against the files
    the reference's gat-run.py wrote for the same inputs and seed (tests/golden/cli/aux/patterns/, make_goldens.py g5)."""
    cli = os.path.join(G, "cli")
    want = os.path.join(cli, "aux", "patterns")
    args = ["--segments=%s" % os.path.join(cli, "segments.bed"), "--annotations=%s" % os.path.join(cli, "annotations.bed"),
            "--workspace=%s" % os.path.join(cli, "workspace.bed"), "--isochores=%s" % os.path.join(cli, "isochores.bed"),
            "--with-segment-tracks", "--num-samples=5", "--random-seed=21", "--counter=nucleotide-overlap",
            "--counter=segment-overlap", "--output-tables-pattern=%s" % str(tmp_path / "table_%s.tsv"),
            "--output-counts-pattern=%s" % str(tmp_path / "counts_%s.tsv"),
            "--output-samples-pattern=%s" % str(tmp_path / "samples_%s.bed")]
    _run_cli(tmp_path, "stdout", args)
    for fn in sorted(os.listdir(want)):
        if fn == "stdout.txt":
            continue
        got = [l for l in open(str(tmp_path / fn)) if not l.startswith("#")]
        assert got == open(os.path.join(want, fn)).readlines(), fn


def test_cli_sample_file_matches_reference(ctx, tmp_path):
    """--sample-file (gat/__init__.py:952-961, Engine.pyx:3215-3233): the files --output-samples-pattern wrote are read
    back (track name = what the pattern's %s matches), no sample file is written by such a run, and the table is the one the
    reference's gat-run.py printed for the same command (tests/golden/cli/aux/expected_sample_file.tsv, make_goldens.py g5s
    -- with the one-token fix of its regex line, build_reference.sh); the reference's two errors are reproduced."""
    import shutil
    cli = os.path.join(G, "cli")
    base = ["--segments=%s" % os.path.join(cli, "segments.bed"), "--annotations=%s" % os.path.join(cli, "annotations.bed"),
            "--workspace=%s" % os.path.join(cli, "workspace.bed"), "--isochores=%s" % os.path.join(cli, "isochores.bed"),
            "--with-segment-tracks", "--num-samples=5", "--random-seed=21", "--counter=nucleotide-overlap"]
    # the sample files: this build's own (equal to the reference's, test_cli_pattern_outputs_match_reference)
    _run_cli(tmp_path, "first", base + ["--output-samples-pattern=%s" % str(tmp_path / "samples_%s.bed")])
    files = [str(tmp_path / "samples_segA.bed"), str(tmp_path / "samples_segB.bed")]
    for f in files:
        assert open(f).read() == open(os.path.join(cli, "aux", "patterns", os.path.basename(f))).read()
    before = [(os.path.getmtime(f), open(f).read()) for f in files]
    got = _run_cli(tmp_path, "second", base + ["--output-samples-pattern=%s" % str(tmp_path / "samples_%s.bed"),
                                               "--sample-file=%s" % str(tmp_path / "samples_seg*.bed")])
    assert got == open(os.path.join(cli, "aux", "expected_sample_file.tsv")).readlines()
    assert [(os.path.getmtime(f), open(f).read()) for f in files] == before          # read, not rewritten
    errors = json.load(open(os.path.join(cli, "aux", "sample_file_errors.json")))
    assert errors == {"no_pattern": "ValueError", "pattern_does_not_match": "AttributeError"}
    with pytest.raises(ValueError):
        _run_cli(tmp_path, "e1", base + ["--sample-file=%s" % files[0]])
    with pytest.raises(AttributeError):
        _run_cli(tmp_path, "e2", base + ["--sample-file=%s" % files[0], "--output-samples-pattern=%s" % str(tmp_path / "other_%s.txt")])
    # a file that is not a bed file raises the bed reader's error, as loading it in the reference does
    shutil.copy(os.path.join(cli, "aux", "descriptions.tsv"), str(tmp_path / "samples_bad.bed"))
    with pytest.raises(Exception):
        _run_cli(tmp_path, "e3", base + ["--sample-file=%s" % str(tmp_path / "samples_bad.bed"),
                                         "--output-samples-pattern=%s" % str(tmp_path / "samples_%s.bed")])


def test_more_units_than_a_grid_dimension(ctx):
    """72 000 isochore units (9 000 contigs x 8 classes), 69 827 of them non-empty: the units' launch index is
    spread over two grid dimensions (about 25 s: the oracle zeroes its 100 000-bin histogram per unit and sample)."""
    import collections
    from gat_amd import problem
    rs = np.random.RandomState(5)
    n_contigs = 9000
    contigs = collections.OrderedDict(("s%05d" % i, 40000) for i in range(n_contigs))
    segs = synthetic.random_segments(contigs, 500000, 60, 321)
    annos = [("t0", synthetic.random_segments(contigs, 30000, 400, 322))]
    ws = synthetic.workspace_ungapped(contigs, pieces=1, gap=200)
    iso = synthetic.isochores_blocks(contigs, nclasses=8, block=2500)
    flat = problem.flatten_arrays(segs, annos, ws, iso)
    assert flat["n_units"] == 72000 and int((flat["unit_contig"] >= 0).sum()) > 65535   # beyond one grid dimension
    counters = ["nucleotide-overlap", "segment-overlap"]
    S = 2
    want, wsamples = O.run_samples(flat, counters, 17, 1, 0, S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 17, 0, S)
    for k in range(len(counters)):
        assert np.array_equal(got[k], want[k])
    seg, off = P.sample(17, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()


def test_more_contigs_than_a_grid_dimension(ctx):
    """70 000 contigs without isochores (units = contigs): the count kernels index (track tile, contig) pairs and the
    contig kernels contigs over two grid dimensions."""
    import collections
    from gat_amd import intervals as iv, problem
    n = 70000
    segs, anno, ws = collections.OrderedDict(), collections.OrderedDict(), collections.OrderedDict()
    for i in range(n):
        k = 3 + i % 4
        st = 5000 + np.arange(k) * 3000 + (i * 37) % 1000
        ln = 40 + (i * 13 + np.arange(k) * 7) % 100
        name = "c%05d" % i
        segs[name] = iv.make(st, st + ln)
        a0 = 4000 + (i * 53) % 3000
        anno[name] = iv.make(np.array([a0, a0 + 9000]), np.array([a0 + 2500, a0 + 12000]))
        ws[name] = iv.make(np.array([200]), np.array([39800]))
    flat = problem.flatten_arrays(segs, [("t0", anno)], ws, None)
    assert flat["n_contigs"] == n > 65535
    counters = ["nucleotide-overlap", "segment-overlap", "annotation-overlap"]
    S = 2
    want, wsamples = O.run_samples(flat, counters, 23, 1, 0, S, want_samples=True)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 23, 0, S)
    for k in range(len(counters)):
        assert np.array_equal(got[k], want[k])
    seg, off = P.sample(23, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    P.close()


def _edge_case(ctx, seed):
    """the corners: segments longer than workspace pieces, one-base pieces, units of one to three segments, dense units
    (overshoot trims, unsuccessful rounds), odd bucket sizes"""
    import collections
    from gat_amd import problem, intervals as iv
    rs = np.random.RandomState(seed)
    contigs = collections.OrderedDict(("e%d" % i, int(rs.randint(3000, 200000))) for i in range(int(rs.randint(1, 4))))
    segs, ws = collections.OrderedDict(), collections.OrderedDict()
    for c, size in contigs.items():
        nseg = int(rs.choice([1, 2, 3, 10, 60, 300]))
        mean = int(rs.choice([1, 5, 50, 500, 3000]))
        st = rs.randint(0, size, nseg)
        ln = 1 + rs.geometric(1.0 / mean, nseg)
        segs[c] = iv.normalize(iv.make(st, np.minimum(st + ln, size + 5000)))
        npieces = int(rs.choice([1, 2, 7, 40]))
        edges = np.sort(rs.choice(np.arange(1, size), size=min(2 * npieces, size - 1), replace=False))
        ws[c] = iv.normalize(iv.make(edges[0::2][:npieces], edges[1::2][:npieces] + int(rs.choice([0, 0, 1]))))
        ws[c] = ws[c][ws[c]["end"] > ws[c]["start"]]
    annos = [("t0", synthetic.random_segments(contigs, int(rs.randint(5, 200)), int(rs.randint(20, 2000)), int(rs.randint(1 << 30))))]
    bucket_size = int(rs.choice([0, 1, 3, 64]))
    nbuckets = int(rs.choice([100000, 5000]))
    try:
        flat = problem.flatten_arrays(segs, annos, ws, None, bucket_size=bucket_size, nbuckets=nbuckets)
    except Exception:                  # noqa: BLE001  (degenerate generator output)
        return "skipped"
    if flat["n_contigs"] == 0:
        return "skipped"
    counters = list(_lib.COUNTER_IDS.keys())
    S = 10
    try:
        want, wsamples = O.run_samples(flat, counters, seed, 1, 0, S, want_samples=True)
    except (ValueError, AssertionError) as e:
        try:
            P = _lib.Problem(ctx, flat)
            P.sample_and_count(counters, seed, 0, S)
        except type(e):
            return "both raised %s" % type(e).__name__
        raise AssertionError("oracle raised %s, the device path did not" % type(e).__name__)
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, seed, 0, S)
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), c
    seg, off = P.sample(seed, 0, S)
    assert np.array_equal(off, wsamples[1]) and np.array_equal(seg, wsamples[0])
    _check_counts_alone(P, counters, want, seed, 0, S)
    P.close()
    return "compared"


@pytest.mark.parametrize("seed", [2614126, 2764763])
def test_lists_that_outgrow_64_times_their_region(ctx, seed):
    """a unit of one 70 000-base segment and one of two bases in a workspace of 40 pieces of 32 000 bases in all: the small one is
    placed tens of thousands of times between the large one's trims, the list grows to 100 times the unit's region -- the library
    doubles the regions until it fits (round 5 gave up at 64 x: two of 200 000 edge-case seeds of round 6's sweep)"""
    assert _edge_case(ctx, seed) == "compared"


@pytest.mark.parametrize("seed", list(range(1, 49)))
def test_fuzz_edge_cases_vs_oracle(ctx, seed):
    """the corners (see _edge_case): equal to the oracle, or the same exception on both sides"""
    assert _edge_case(ctx, seed) in ("compared", "skipped", "both raised ValueError", "both raised AssertionError")


@pytest.mark.parametrize("seed", list(range(300, 316)))
def test_merged_track_index_vs_oracle(ctx, seed, monkeypatch):
    """k_count_merged (nucleotide counters against several tracks through one merged, position-gridded index of all
    tracks): forced on from one track up, on shapes that stress it -- intervals far longer than the piece bound (cut into
    pieces), tracks that overlap each other heavily, empty tracks / contigs, isochores, dense sample lists -- against the
    oracle, and against the per-track kernel on the same problem."""
    import collections
    from gat_amd import problem, intervals as iv
    monkeypatch.setitem(ctx.options, "GAT_MERGED_MIN_TRACKS", "1")
    # the three forms of the scan: index entries fetched in 64-byte blocks of eight / in pairs / the first two out of the
    # grid cell's record (the host picks by the expected length of a scan; here the seed does)
    monkeypatch.setitem(ctx.options, "GAT_MERGED_BLOCK", ("8", "2", "1")[seed % 3])
    rs = np.random.RandomState(seed)
    contigs = collections.OrderedDict(("m%d" % i, int(rs.randint(100000, 2000000))) for i in range(int(rs.randint(1, 4))))
    segs = synthetic.random_segments(contigs, int(rs.choice([40, 400, 3000])), int(rs.choice([30, 300, 2000])), int(rs.randint(1 << 30)))
    n_tracks = int(rs.choice([1, 3, 17, 60]))
    annos = []
    for t in range(n_tracks):
        per = synthetic.random_segments(contigs, int(rs.randint(1, 500)), int(rs.choice([20, 500, 5000])), int(rs.randint(1 << 30)))
        if t % 5 == 1:                                    # a few giants: far beyond 8 x the mean length
            for c, size in contigs.items():
                a0 = int(rs.randint(0, size // 2))
                per[c] = iv.normalize(np.concatenate([per.get(c, iv.EMPTY), iv.make([a0], [a0 + size // 3])]))
        if t % 7 == 3:
            per = collections.OrderedDict()               # an empty track
        annos.append(("t%d" % t, per))
    ws = synthetic.workspace_ungapped(contigs, pieces=int(rs.choice([1, 4])), gap=500)
    iso = synthetic.isochores_blocks(contigs, nclasses=3, block=40000) if seed % 3 == 0 else None
    flat = problem.flatten_arrays(segs, annos, ws, iso)
    counters = ["nucleotide-overlap", "nucleotide-density"]
    S = 6
    try:
        want, _ = O.run_samples(flat, counters, 400 + seed, 1, 0, S)
    except ValueError:                                   # a segment longer than nbuckets * bucket_size
        with pytest.raises(ValueError):
            _lib.Problem(ctx, flat)
        return
    P = _lib.Problem(ctx, flat)
    got = P.sample_and_count(counters, 400 + seed, 0, S)
    assert _lib.COUNT_KERNELS[P.last_stats["count_kernel"]] == "k_count_merged"
    for k, c in enumerate(counters):
        assert np.array_equal(got[k], want[k]), (c, n_tracks)
    monkeypatch.setitem(ctx.options, "GAT_COUNT_NO_MERGED", "1")
    other = P.sample_and_count(counters, 400 + seed, 0, S)
    assert _lib.COUNT_KERNELS[P.last_stats["count_kernel"]] != "k_count_merged"
    for k in range(2):
        assert np.array_equal(other[k], want[k])
    P.close()
    # observed counts (gat_count_lists) take the same kernel
    monkeypatch.delitem(ctx.options, "GAT_COUNT_NO_MERGED")
    C = flat["n_contigs"]
    lists = [flat["segs"][flat["seg_off"][u]:flat["seg_off"][u + 1]] for u in range(flat["n_units"])]
    if iso is None and C == flat["n_units"]:
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        got = ctx.count_lists(counters, np.concatenate(lists), off, 1, flat["annos"], flat["anno_off"], flat["n_tracks"],
                              flat["cws_nseg"], C)
        for t in range(flat["n_tracks"]):
            vals = [O.counter("nucleotide-overlap", lists[c], flat["annos"][flat["anno_off"][t * C + c]:flat["anno_off"][t * C + c + 1]])
                    for c in range(C)]
            assert got[0][t, 0] == int(sum(vals))


def test_point_annotations_errors_like_the_reference(ctx, tmp_path):
    """--annotations-to-points: the three tables in tests/golden/cli/expected_points_*.tsv are compared by
    test_cli_table_matches_reference; here what the reference cannot do with a PositionList (probed on the scratch
    build): any other counter (TypeError in computeCounts, gat/Engine.pyx:2200), isochores (TypeError in fromIsochores,
    :2866) and --truncate-workspace-to-annotations (TypeError in merge, :3007); and the observed counts of the point
    counters against a direct count of positions inside segments."""
    import gat_amd as gat
    from gat_amd import IO
    cli = os.path.join(G, "cli")
    base = ["--segments=%s" % os.path.join(cli, "segments.bed"), "--annotations=%s" % os.path.join(cli, "annotations.bed"),
            "--workspace=%s" % os.path.join(cli, "workspace.bed"), "--num-samples=4", "--random-seed=2",
            "--annotations-to-points=midpoint"]
    for extra in (["--counter=nucleotide-overlap"], ["--counter=segment-overlap"],
                  ["--counter=annotation-overlap", "--isochores=%s" % os.path.join(cli, "isochores.bed")],
                  ["--counter=annotation-overlap", "--truncate-workspace-to-annotations"]):
        with pytest.raises(TypeError):
            _run_cli(tmp_path, "points_err", base + extra)
    opts, _ = gat.buildParser().parse_args(base + ["--counter=annotation-overlap"])
    segments, annotations, workspaces, isochores = IO.buildSegments(opts)
    workspace = IO.applyIsochores(segments, annotations, workspaces, opts, isochores)
    observed = gat.computeCounts(gat.CounterAnnotationOverlap(), sum, segments, annotations, workspace, gat.UnconditionalWorkspace())
    for track in annotations.tracks:
        want = 0
        for contig in workspace.keys():
            seg = segments["merged"][contig].asArray()
            for p in annotations[track][contig].asList():
                want += int(((seg["start"] <= p) & (p < seg["end"])).any())
        assert observed["merged"][track] == want and want > 0


@pytest.mark.parametrize("S", [1, 5, 8, 77, 128, 129, 1000, 8192, 8193, 20011])
def test_device_null_stats_equal_numpy(ctx, S):
    """gat_null_stats (mean, std, interval values, counts below / equal to the observed value, from the device count
    matrix) against what AnnotatorResult computes with numpy on the host, bit for bit: integer rows with heavy ties,
    double rows (density), observed values inside, below and above the distribution, and the reference's p-value known
    answers of tests/golden/stats.json run through the device path."""
    import gat_amd
    rs = np.random.RandomState(S)
    rows = []
    rows.append(rs.randint(0, 50, S).astype(np.int64))                      # ties everywhere
    rows.append(rs.randint(0, 10 ** 7, S).astype(np.int64))
    rows.append((rs.random_sample(S) * 1e5).view(np.int64))                 # IEEE doubles (density)
    rows.append(np.full(S, 7, dtype=np.int64))                              # constant
    rows.append(np.abs(rs.standard_cauchy(S) * 1e3).view(np.int64))         # heavy tail, doubles
    is_double = np.array([0, 0, 1, 0, 1], dtype=np.uint8)
    mat = np.ascontiguousarray(np.stack(rows))
    as_float = [r.view(np.float64) if d else r.astype(np.float64) for r, d in zip(rows, is_double)]
    vals = np.array([float(np.median(as_float[0])), -1.0, float(as_float[2][0]), 7.0, 1e12])
    dev = ctx.alloc(mat.nbytes)
    try:
        _lib._check(_lib.lib().gat_memcpy_h2d(ctx._h, dev, mat.ctypes.data, mat.nbytes), ctx._h)
        st = ctx.null_stats(dev, len(rows), S, is_double, vals)
    finally:
        ctx.free(dev)
    for r in range(len(rows)):
        host = gat_amd.AnnotatorResult("t", "a", "c", vals[r], as_float[r])
        devr = gat_amd.AnnotatorResult("t", "a", "c", vals[r], as_float[r], _stats=tuple(st[r, :6]))
        for f in ("expected", "stddev", "lower95", "upper95", "fold", "pvalue"):
            assert getattr(host, f) == getattr(devr, f), (S, r, f, getattr(host, f), getattr(devr, f))
        assert str(host) == str(devr)


def test_device_null_stats_golden_and_run(ctx, monkeypatch):
    """the reference's statistics goldens (tests/golden/stats.json, incl. its p-value known answers) through the device
    path, and gat_amd.run() with GAT_DEVICE_STATS=1 against the rows the reference printed (run_small_isochores)."""
    import gat_amd
    with open(os.path.join(G, "stats.json")) as f:
        cases = [c for c in json.load(f) if "reference_fold" not in c]
    for c in cases:
        samples = np.array(c["samples"], dtype=np.float64)
        mat = samples.view(np.int64).reshape(1, -1).copy()
        dev = ctx.alloc(mat.nbytes)
        try:
            _lib._check(_lib.lib().gat_memcpy_h2d(ctx._h, dev, mat.ctypes.data, mat.nbytes), ctx._h)
            st = ctx.null_stats(dev, 1, len(samples), np.array([1], dtype=np.uint8), np.array([c["observed"]]))
        finally:
            ctx.free(dev)
        host = gat_amd.AnnotatorResult("t", "a", "c", c["observed"], samples, pseudo_count=c["pseudo_count"])
        devr = gat_amd.AnnotatorResult("t", "a", "c", c["observed"], samples, pseudo_count=c["pseudo_count"], _stats=tuple(st[0, :6]))
        assert str(host) == str(devr)
        for key in ("expected", "stddev", "pvalue", "fold"):
            if key in c:
                assert getattr(devr, key) == c[key], key
    monkeypatch.setenv("GAT_DEVICE_STATS", "1")
    test_run_api_rows_match_reference(ctx)


@pytest.mark.parametrize("with_isochores", [True, False])
def test_grouped_annotation_lists_equal_contig_lists(ctx, with_isochores):
    """gat_problem_desc::anno_group: the annotation lists handed over one per (track, key) with a group id each -- the
    library forms the contig-level lists (IntervalDictionary.fromIsochores, gat/Engine.pyx:2857-2876) on its host threads --
    against the same problem described with the contig-level lists made by the host (problem.flatten_units), and both
    against the oracle: all six counters, isochore keys (concatenate, sort, merge(0)) and plain keys (pass through)."""
    from gat_amd import problem, synthetic
    _, cfg = synthetic.small_genome()
    if not with_isochores:
        cfg["isochores"] = None
    segments, annotations, workspace, _ = synthetic.as_collections(cfg)
    if not with_isochores:
        for coll in (segments, annotations):             # gat/IO.py:243-248 without isochores
            for t in coll.tracks:
                for c in list(coll[t].keys()):
                    if c in workspace:
                        coll[t][c].intersect(workspace[c])
                    else:
                        del coll[t][c]
    segs = segments["merged"]
    tracks = list(annotations.tracks)
    new = problem.flatten_dictionaries(segs, workspace, annotations, tracks, 1, 1000)
    old = problem.flatten_units(segs.asArrays(), workspace.asArrays(), [(t, annotations[t].asArrays()) for t in tracks], 1, 1000)
    assert new is not None and new["merge_contigs"] == (1 if with_isochores else 0)
    counters = list(_lib.COUNTER_IDS.keys())
    Pn, Po = _lib.Problem(ctx, new), _lib.Problem(ctx, old)
    got_n = Pn.sample_and_count(counters, 77, 3, 19)
    got_o = Po.sample_and_count(counters, 77, 3, 19)
    want, _ = O.run_samples(old, counters, 77, 1, 3, 19)
    for k, c in enumerate(counters):
        assert np.array_equal(got_n[k], got_o[k]), c
        assert np.array_equal(got_n[k], want[k]), c
    Pn.close()
    Po.close()


def test_count_list_ranges_equals_csr(ctx):
    """gat_count_list_ranges: the annotation lists as ranges of one array, in any order and with gaps, against the CSR form"""
    rs = np.random.RandomState(19)
    n_groups, n_tracks, n_lists = 4, 5, 2
    mk = lambda n, w: np.array(O.normalize([(int(a), int(a + b)) for a, b in zip(rs.randint(0, 60000, n), rs.randint(1, w, n))]), dtype=_lib.SEG)  # noqa: E731
    lists = [mk(70, 300) for _ in range(n_lists * n_groups)]
    annos = [mk(50, 900) if i % 7 else mk(0, 2) for i in range(n_tracks * n_groups)]
    off = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)  # noqa: E731
    ws_nseg = [3, 1, 7, 2]
    counters = list(_lib.COUNTER_IDS.keys())
    want = ctx.count_lists(counters, np.concatenate(lists), off(lists), n_lists, np.concatenate(annos), off(annos), n_tracks, ws_nseg, n_groups)
    order = rs.permutation(len(annos))                   # the array holds the lists in another order, with filler between
    filler = mk(5, 10)
    pieces, begin, end, pos = [], np.zeros(len(annos), np.int64), np.zeros(len(annos), np.int64), 0
    for i in order:
        pieces.append(filler)
        pos += len(filler)
        begin[i], end[i] = pos, pos + len(annos[i])
        pieces.append(annos[i])
        pos += len(annos[i])
    got = ctx.count_lists(counters, np.concatenate(lists), off(lists), n_lists, np.concatenate(pieces), begin, n_tracks, ws_nseg, n_groups,
                          anno_end=end)
    for k in range(len(counters)):
        assert np.array_equal(got[k], want[k]), counters[k]
