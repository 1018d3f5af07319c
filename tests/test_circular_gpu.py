"""GPU: SamplerCircular (k_circular) through the C ABI and the Python layers against tests/circular_model.py, list for list:
random units, the wave-step carries, the edges of the rotation (each reached by a seed found on the model and asserted
there), both ends of the coordinate range, and the sampler's consumers."""
import importlib.util
import os
import random

import numpy as np
import pytest

import circular_cases as CIRC
import circular_model as M
import coverage_cases as CC
import coverage_model
import gat_amd
from circular_cases import EDGE_SEGS, EDGE_WS, rand_norm, unit_of_n, units_flat
from gat_amd import _lib, problem, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCULAR = 6
INT_COUNTERS = ["nucleotide-overlap", "segment-overlap", "segment-midoverlap", "annotation-overlap", "annotation-midoverlap"]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
def as_lists(seg, off):
    s, e = seg["start"].tolist(), seg["end"].tolist()
    return [list(zip(s[off[i]:off[i + 1]], e[off[i]:off[i + 1]])) for i in range(len(off) - 1)]


def device_units(ctx, flat, seed, s0, s1):
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(seed, s0, s1, unit_level=True)
        return as_lists(seg, off), P.last_stats
    finally:
        P.close()


def check_units(ctx, units, seed, s0, s1, info=None):
    """the device's (sample, unit) lists and its draw count against the model's"""
    flat = units_flat(units)
    want, ndraws = M.model_units(flat, seed, s0, s1, info)
    got, st = device_units(ctx, flat, seed, s0, s1)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i // len(units), i % len(units), g[:6], w[:6])
    assert st["n_draws"] == ndraws
    return want


# ------------------------------------------------------------------------------------------------ random units
def random_units(r, n):
    units = []
    for _ in range(n):
        span = r.choice([200, 1000, 5000, 40000])
        segs = rand_norm(r, r.randint(1, 14), span, r.choice([1, 5, 50, 400, 3000]))
        if r.random() < 0.33:     # fragmented workspace: hundreds of short pieces, touching ones among them
            n_ws = r.randint(100, 400)
            ws = rand_norm(r, n_ws, max(span, 6 * n_ws) + 100, r.choice([2, 5, 20]))
        else:
            ws = rand_norm(r, r.randint(1, 20), span + 100, r.choice([1, 3, 30, 2000]))
        units.append((segs, ws))
    return units


RANDOM_UNITS = random_units(random.Random(0xC1CC), 80)


@pytest.mark.parametrize("seed", [1234, 7, 2 ** 32 - 3])
def test_random_units(ctx, seed):
    """80 random units, a third with fragmented workspaces, x 6 samples (seed 2^32 - 3: the unit streams' seeds wrap)"""
    info = []
    check_units(ctx, RANDOM_UNITS, seed, 0, 6, info)
    assert sum(1 for st in info if st["r"] is not None) > 300


def test_split_sample_range(ctx):
    flat = units_flat(RANDOM_UNITS)
    whole, _ = device_units(ctx, flat, 99, 0, 13)
    part, _ = device_units(ctx, flat, 99, 5, 13)
    assert part == whole[5 * len(RANDOM_UNITS):]
    assert whole == M.model_units(flat, 99, 0, 13)[0]


# ------------------------------------------------------------------------------------------------ wave-step carries
@pytest.mark.parametrize("frag", [False, True])
def test_wave_step_sizes(ctx, frag):
    r = random.Random(64 + frag)
    units = []
    for n in (1, 63, 64, 65, 128, 129):
        u, n_iv = unit_of_n(r, n, False)
        assert n_iv == n
        units.append(unit_of_n(r, n, True)[0] if frag else u)
    check_units(ctx, units, 5, 0, 8)


def test_long_unit_beside_a_short_one(ctx):
    r = random.Random(2500)
    long_unit, n_iv = unit_of_n(r, 2500, False)
    assert n_iv == 2500
    check_units(ctx, [long_unit, ([(3, 9)], [(0, 20)])], 11, 0, 4)


# ------------------------------------------------------------------------------------------------ edges
def _edge(ctx, units, seed, unit=0):
    """sample 0 of the units under `seed`: the model's stats of `unit` and its list, after the device agreed"""
    info = []
    want = check_units(ctx, units, seed, 0, 1, info)
    return info[unit], want[unit]


def test_edge_interval_ends_at_wsum(ctx):
    st, _ = _edge(ctx, [(EDGE_SEGS, EDGE_WS)], 3)
    assert st["wsum"] == 36 and st["r"] > 0 and any(b + st["r"] in (36, 72) for a, b in M.linear_intervals(EDGE_SEGS, EDGE_WS))


def test_edge_r_zero_returns_the_working_list(ctx):
    st, got = _edge(ctx, [(EDGE_SEGS, EDGE_WS)], 0)
    assert st["r"] == 0 and got == [(12, 15), (18, 20), (25, 27), (50, 60)]


def test_edge_interval_starts_at_the_wrap(ctx):
    st, got = _edge(ctx, [(EDGE_SEGS, EDGE_WS)], 6)
    assert any(a + st["r"] == 36 for a, b in M.linear_intervals(EDGE_SEGS, EDGE_WS)) and got[0][0] == 10


def test_edge_interval_cut_by_the_wrap(ctx):
    st, got = _edge(ctx, [(EDGE_SEGS, EDGE_WS)], 4)
    assert any(a + st["r"] < 36 < b + st["r"] for a, b in M.linear_intervals(EDGE_SEGS, EDGE_WS))
    assert got[0][0] == 10 and got[-1][1] == 60


def test_edge_interval_over_three_pieces(ctx):
    st, got = _edge(ctx, [(EDGE_SEGS, EDGE_WS)], 1)
    r = st["r"]
    assert any(len(M.rotate([iv], EDGE_WS, r)) >= 3 for iv in M.linear_intervals(EDGE_SEGS, EDGE_WS))


def test_edge_pieces_of_one_base(ctx):
    ws = [(2 * i, 2 * i + 1) for i in range(90)] + [(200, 201), (201, 202), (202, 203)]
    segs = [(4, 31), (60, 61), (100, 140), (199, 203)]
    info = []
    check_units(ctx, [(segs, ws)], 3, 0, 8, info)
    assert info[0]["wsum"] == 93 and len({st["r"] for st in info}) > 4


def test_edge_wsum_one(ctx):
    info = []
    want = check_units(ctx, [([(5, 9)], [(7, 8)]), ([(0, 3)], [(0, 10)])], 12, 0, 3, info)
    assert info[0]["wsum"] == 1 and info[0]["r"] == 0 and want[0] == [(7, 8)]


def test_edge_one_piece_filled_by_one_segment(ctx):
    st, got = _edge(ctx, [([(90, 200)], [(100, 110)])], 0)
    assert st["n"] == 1 and st["r"] > 0
    assert got == [(100, 100 + st["r"]), (100 + st["r"], 110)]          # two touching pieces, kept apart


def test_edge_one_and_a_thousand_workspace_pieces(ctx):
    r = random.Random(1000)
    ws = [(5 * i, 5 * i + r.choice((1, 3, 5))) for i in range(1000)]
    segs = [(0, 4), (40, 900), (1000, 1001), (2000, 4990), (4996, 5000)]
    info = []
    want = check_units(ctx, [(segs, ws), (segs, [(0, 5000)])], 8, 0, 6, info)
    assert max(len(x) for x in want) > 500 and info[1]["wsum"] == 5000


def test_edge_unit_without_working_segments(ctx):
    units = [([(3, 9)], [(0, 20)]), ([(500, 510)], [(0, 100)]), ([], [(0, 10)]), ([(1, 2)], []), ([(30, 45)], [(10, 40), (44, 50)])]
    want = check_units(ctx, units, 4, 0, 5)
    assert all(want[s * 5 + u] == [] for s in range(5) for u in (1, 2, 3)) and all(want[s * 5 + 4] for s in range(5))


# ------------------------------------------------------------------------------------------------ whole problems
def genome_flat(isochores):
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"] if isochores else None)
    flat["sampler"] = CIRCULAR
    return flat


def counts_of_lists(ctx, flat, unit_lists, counters, S):
    """the counters over the contig lists of the (sample, unit) lists -- the units of a contig concatenated and merge(0)d when
    the keys carry isochores -- through gat_count_lists: [counter][track, sample]"""
    n, nc = int(flat["n_units"]), int(flat["n_contigs"])
    lists = []
    for s in range(S):
        contig = [[] for _ in range(nc)]
        for u in range(n):
            c = int(flat["unit_contig"][u])
            if c >= 0:
                contig[c] += unit_lists[s * n + u]
        if int(flat["merge_contigs"]):
            contig = [O.aslist(O.merge(sorted(x), 0)) if x else [] for x in contig]
        lists += contig
    cat = np.zeros(sum(len(x) for x in lists), dtype=O.SEG)
    k = 0
    for x in lists:
        for a, b in x:
            cat[k] = (a, b)
            k += 1
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return ctx.count_lists(counters, cat, off, S, flat["annos"], flat["anno_off"], int(flat["n_tracks"]), flat["cws_nseg"], nc)


@pytest.mark.parametrize("isochores", [False, True])
def test_problem_lists_and_counts(ctx, isochores):
    """a whole problem (with isochores: several units per contig): the unit lists, and the count matrices of
    gat_sample_and_count against the model's lists counted by gat_count_lists; a split sample range gives the same"""
    flat = genome_flat(isochores)
    S = 12
    want_lists, _ = M.model_units(flat, 77, 0, S)
    assert device_units(ctx, flat, 77, 0, S)[0] == want_lists
    if isochores:
        units_per_contig = np.bincount(np.asarray(flat["unit_contig"])[np.asarray(flat["unit_contig"]) >= 0])
        assert units_per_contig.max() > 1
    want = counts_of_lists(ctx, flat, want_lists, INT_COUNTERS, S)
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(INT_COUNTERS, 77, 0, S)
        parts = [P.sample_and_count(INT_COUNTERS, 77, a, b) for a, b in ((0, 5), (5, 12))]
        state = np.zeros(_lib.MT_STATE_WORDS, dtype=np.uint32)
        state[-1] = 624
        with pytest.raises(Exception, match="SamplerCircular runs on the per-unit streams only"):
            P.sample_and_count_serial(INT_COUNTERS, state, 4)
    finally:
        P.close()
    for k, c in enumerate(INT_COUNTERS):
        assert np.array_equal(got[k], want[k]), c
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), want[k]), c


CONSUMER_PROBLEMS = dict({name: CC.SIX[name] for name in CC.CIRCULAR_NAMES}, **{"dense-isochores": CIRC.dense_isochore_problem})


@pytest.mark.parametrize("name", sorted(CONSUMER_PROBLEMS))
def test_consumer_problems_sample_is_the_models(ctx, name):
    """what every list consumer reads, for the problems their tests run on (tests/coverage_cases.py: SIX) under their seed and
    samples: the unit lists, and the contig lists -- with isochore keys k_contig's merged lists (d_cslab): the model's unit
    lists of a contig one after the other and merge(0)d"""
    flat = CONSUMER_PROBLEMS[name]()
    want_units, want_off = CIRC.model_sample(flat, CIRC.SEED, 0, CIRC.SAMPLES, unit_level=True)
    want, off = CIRC.model_sample(flat, CIRC.SEED, 0, CIRC.SAMPLES)
    P = _lib.Problem(ctx, flat)
    try:
        got_units, got_unit_off = P.sample(CIRC.SEED, 0, CIRC.SAMPLES, unit_level=True)
        got, got_off = P.sample(CIRC.SEED, 0, CIRC.SAMPLES)
        part, part_off = P.sample(CIRC.SEED, 5, CIRC.SAMPLES)
    finally:
        P.close()
    assert got_unit_off.tolist() == want_off.tolist() and got_units.tolist() == want_units.tolist()
    assert got_off.tolist() == off.tolist() and got.tolist() == want.tolist()
    at = 5 * int(flat["n_contigs"])
    assert (part_off + off[at]).tolist() == off[at:].tolist() and part.tolist() == want[off[at]:].tolist()
    if int(flat["merge_contigs"]):
        assert int(flat["n_units"]) > int(flat["n_contigs"])
        assert (len(want) < len(want_units)) == (name == "dense-isochores")         # (touching unit pieces, united)


def test_run_counts(ctx, monkeypatch):
    """gat_amd.run(sampler=SamplerCircular()): every result's samples are the model's lists counted by gat_count_lists"""
    _, cfg = synthetic.small_genome()
    cfg = dict(cfg, isochores=None)
    segments, annotations, workspace, _ = synthetic.as_collections(cfg)
    flats = []
    init = _lib.Problem.__init__

    def recording(self, c, flat, *args, **kwargs):
        flats.append(flat)
        return init(self, c, flat, *args, **kwargs)
    monkeypatch.setattr(_lib.Problem, "__init__", recording)
    S = 10
    results = gat_amd.run(segments, annotations, workspace, gat_amd.SamplerCircular(), [gat_amd.COUNTERS[c]() for c in INT_COUNTERS],
                          gat_amd.UnconditionalWorkspace(), num_samples=S, random_seed=31)
    assert len(flats) == 1 and int(flats[0]["sampler"]) == CIRCULAR
    units = flats[0]                                            # (the units as run() laid them out)
    names = list(units["contig_names"])
    tracks = [t for t, _ in cfg["annotations"]]
    per = [[a.get(c, np.zeros(0, dtype=O.SEG)) for c in names] for _, a in cfg["annotations"]]
    flat = dict(units, n_tracks=len(tracks), annos=np.concatenate([x for t in per for x in t]),
                anno_off=np.concatenate([[0], np.cumsum([len(x) for t in per for x in t])]).astype(np.int64))
    want_lists, _ = M.model_units(flat, 31, 0, S)
    assert any(want_lists)
    want = counts_of_lists(ctx, flat, want_lists, INT_COUNTERS, S)
    assert len(results) == len(tracks) * len(INT_COUNTERS)
    for r in results:
        k, t = INT_COUNTERS.index(r.counter), tracks.index(r.annotation)
        assert [int(v) for v in r.samples.tolist()] == want[k][t].tolist(), (r.counter, r.annotation)


CLI = os.path.join(ROOT, "tests", "golden", "cli")


def test_null_round_size_gives_the_plain_runs_rows():
    """--null-round-size with --sampler=circular: the rounds' words are those of the samples the plain run kept"""
    import null_fold_model as NF
    counters = ["nucleotide-overlap", "segment-overlap"]

    def rows(null_round_size):
        argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
                "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=60", "--random-seed=5", "--sampler=circular",
                "--null-round-size=%d" % null_round_size] + ["--counter=%s" % c for c in counters]
        options, args = gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS).parse_args(argv)
        return gat_amd.fromSegments(options, args)
    plain, deep = rows(0), rows(7)
    assert len(plain) == len(deep) >= 2 * len(counters)
    for p, d in zip(plain, deep):
        assert (p.track, p.annotation, p.counter, p.observed) == (d.track, d.annotation, d.counter, d.observed)
        assert d.null_words == NF.row_words([int(v) for v in p.samples.tolist()], p.observed), (d.counter, d.annotation)
        assert (d.nsamples, d.expected, d.pvalue, d.fold) == (60, p.expected, p.pvalue, p.fold)
        assert str(d).split("\t")[7:] == str(p).split("\t")[7:]
    assert len({tuple(p.samples.tolist()) for p in plain}) > 1                 # (the null is not one constant row)


def test_coverage_script_per_base(tmp_path):
    """gat-coverage --sampler=circular --bin-size=1 on a workspace of 37 bases in 3 pieces: the model's per-base counts"""
    ws = [(10, 20), (25, 40), (50, 62)]
    segs = [(12, 18), (19, 27), (38, 52), (60, 70)]
    assert M.workspace_sum(ws) == 37
    (tmp_path / "s.bed").write_text("".join("chr1\t%d\t%d\n" % x for x in segs))
    (tmp_path / "w.bed").write_text("".join("chr1\t%d\t%d\n" % x for x in ws))
    spec = importlib.util.spec_from_file_location("gat_coverage_cli_circular", os.path.join(ROOT, "scripts", "gat-coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "coverage.tsv"
    S = 25
    assert mod.main(["gat-coverage.py", "--stdout=%s" % out, "--segments=%s" % (tmp_path / "s.bed"), "--workspace=%s" % (tmp_path / "w.bed"),
                     "--num-samples=%d" % S, "--random-seed=9", "--bin-size=1", "--sampler=circular", "--verbose=0"]) == 0
    lines = open(str(out)).read().splitlines()
    assert not [l for l in lines[1:] if l.startswith("#")]                     # (nothing sampled beyond the last bin)
    rows = {int(f[2]): [int(x) for x in f[4:9]] for f in (l.split("\t") for l in lines[1:])}
    n_bins = 62
    bases, starts, ends = (np.zeros(n_bins, dtype=np.int64) for _ in range(3))
    rs = set()
    for s in range(S):                                                         # one unit: sample s draws from seed 9 + s
        st = {}
        lst = M.sample(O.RandomState(9 + s), segs, ws, st)
        rs.add(st["r"])
        b, a, e, outside = coverage_model.coverage_naive(lst, 1, n_bins)
        assert outside == 0 and b.sum() == 6 + 3 + 4 + 2
        bases, starts, ends = bases + b, starts + a, ends + e
    assert len(rs) > 10
    in_ws = {x for a, b in ws for x in range(a, b)}
    assert set(rows) == in_ws
    for x in sorted(in_ws):
        assert rows[x] == [1, int(any(a <= x < b for a, b in segs)), bases[x], starts[x], ends[x]], x


def test_sampler_class(ctx):
    """SamplerCircular.sample: numpy's seed convention, an isNormalized result, an empty list without working segments"""
    def slist(pairs):
        a = np.zeros(len(pairs), dtype=O.SEG)
        for i, p in enumerate(pairs):
            a[i] = p
        s = gat_amd.SegmentList(array=a)
        s.isNormalized = 1
        return s
    s = gat_amd.SamplerCircular()
    for seed in (0, 5, 2 ** 32 - 1):
        got = s.sample(slist(EDGE_SEGS), slist(EDGE_WS), seed=seed)
        assert got.isNormalized and [tuple(int(v) for v in x) for x in got] == M.sample(O.RandomState(seed), EDGE_SEGS, EDGE_WS)
    np.random.seed(3)
    seed = int(np.random.randint(0, 2 ** 32))
    np.random.seed(3)
    got = s.sample(slist(EDGE_SEGS), slist(EDGE_WS))
    assert [tuple(int(v) for v in x) for x in got] == M.sample(O.RandomState(seed), EDGE_SEGS, EDGE_WS)
    assert len(s.sample(slist([(100, 120)]), slist(EDGE_WS), seed=1)) == 0


# ------------------------------------------------------------------------------------------------ coordinate range
def test_one_piece_of_three_billion_bases(ctx):
    """[0, 3 * 10^9) with segments near both ends: a + r passes 2^32, positions need 64 bits"""
    ws = [(0, 3_000_000_000)]
    segs = [(5, 17), (1000, 1001), (2_999_999_000, 2_999_999_500), (2_999_999_990, 3_000_000_000)]
    info = []
    want = check_units(ctx, [(segs, ws)], 21, 0, 8, info)
    assert any(2_999_999_000 + st["r"] >= 2 ** 32 for st in info) and any(st["r"] < 2 ** 31 for st in info)
    assert all(sum(b - a for a, b in x) == 12 + 1 + 500 + 10 for x in want)


def test_workspace_above_two_to_the_31(ctx):
    base = 2 ** 31
    ws = [(base + 100, base + 5000), (base + 6000, base + 9000), (2 ** 32 - 50, 2 ** 32 - 1)]
    segs = [(base + 90, base + 130), (base + 4990, base + 6010), (base + 8000, base + 8100), (2 ** 32 - 60, 2 ** 32 - 10)]
    info = []
    want = check_units(ctx, [(segs, ws)], 6, 0, 8, info)
    assert all(a >= base + 100 for x in want for a, b in x) and len({st["r"] for st in info}) == 8
