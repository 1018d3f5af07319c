"""GPU: SamplerUniverse (k_universe) through the C ABI and the Python layers against tests/universe_model.py, list for list: the
ends of the draw (m = 1, k = 0, k = m), the complement switch, the mark table's word and wave-step edges, units of unequal
size in one launch, isochore units, split sample ranges, more units than a grid dimension, and the sampler's consumers."""
import importlib.util
import os
import random

import numpy as np
import pytest

import circular_cases as CIRC
import coverage_model
import gat_amd
import universe_cases as UC
import universe_model as M
from gat_amd import _lib, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ["nucleotide-overlap", "segment-overlap"]


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
    flat = UC.units_flat(units)
    want, ndraws = M.model_units(flat, seed, s0, s1, info)
    got, st = device_units(ctx, flat, seed, s0, s1)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i // len(units), i % len(units), len(g), len(w), g[:6], w[:6])
    assert st["n_draws"] == ndraws
    return want


# ------------------------------------------------------------------------------------------------ the ends of the draw
def test_ends_of_the_draw(ctx):
    """m = 1; k = 0 beside active units; k = m; the single hit piece the first or the last of W"""
    r = random.Random(1)
    w9 = UC.pieces(r, 9)
    units = [
        ([(0, 5)], [(0, 5)]),                                   # m == 1
        ([(w9[-1][1] + 5, w9[-1][1] + 9)], w9),                 # k == 0: the segment lies beyond the universe
        (list(w9), w9),                                         # k == m
        ([w9[0]], w9),                                          # the first piece alone
        ([w9[-1]], w9),                                         # the last piece alone
        ([], w9),                                               # no segments
        ([(w9[2][0], w9[3][1])], w9),                           # one segment over two pieces: k == 2
        UC.unit_of(r, 2, 1),
    ]
    info = []
    want = check_units(ctx, units, 3, 0, 40, info)
    n = len(units)
    assert [info[u]["k"] for u in range(n)] == [1, 0, 9, 1, 1, 0, 2, 1]
    for s in range(40):
        assert want[s * n] == [(0, 5)] and want[s * n + 1] == [] and want[s * n + 2] == w9 and want[s * n + 5] == []
    # over 40 samples the single piece is drawn at both ends of W and in between
    for u in (3, 4):
        drawn = {want[s * n + u][0] for s in range(40)}
        assert w9[0] in drawn and w9[-1] in drawn and len(drawn) > 4


def test_complement_switch(ctx):
    """2k = m, 2k = m - 1 and 2k = m + 1, and the sizes next to them"""
    r = random.Random(2)
    units = [UC.unit_of(r, m, k) for m, k in ((6, 3), (7, 3), (7, 4), (6, 2), (6, 4), (2, 1), (3, 1), (3, 2), (100, 50), (101, 50), (101, 51))]
    info = []
    want = check_units(ctx, units, 11, 0, 12, info)
    assert [(st["c"], st["invert"]) for st in info[:len(units)]] == [(3, False), (3, False), (3, True), (2, False), (2, True), (1, False), (1, False),
                                                                     (1, True), (50, False), (50, False), (50, True)]
    assert all(len(want[i]) == info[i]["k"] for i in range(len(want)))
    assert len({tuple(want[s * len(units)]) for s in range(12)}) > 4           # (the draws differ from sample to sample)


@pytest.mark.parametrize("m", [31, 32, 33, 63, 64, 65])
def test_table_word_edges(ctx, m):
    """the last word of the mark table full, one bit short, one bit over: k = 1, m / 2, m - 1, and the last piece alone"""
    r = random.Random(m)
    units = [UC.unit_of(r, m, k) for k in (1, m // 2, m // 2 + 1, m - 1, m)] + [UC.unit_of(r, m, 1, hit=[m - 1]), UC.unit_of(r, m, 2, hit=[0, m - 1])]
    info = []
    want = check_units(ctx, units, 5, 0, 10, info)
    n = len(units)
    # the unit that leaves one piece out leaves out the last one in some sample, and keeps it in another
    last = [units[3][1][-1] in want[s * n + 3] for s in range(10)] + [units[1][1][-1] in want[s * n + 1] for s in range(10)]
    assert any(last) and not all(last)


@pytest.mark.parametrize("m", [2047, 2048, 2049, 4097])
def test_wave_step_edges(ctx, m):
    """64 words -- 2 048 pieces -- per wave step of the write-out: the carry from step to step, the last step of one piece"""
    r = random.Random(m)
    units = [UC.unit_of(r, m, k) for k in (1, m // 2, m - 1)]
    info = []
    want = check_units(ctx, units, 9, 0, 3, info)
    assert [st["k"] for st in info[:3]] == [1, m // 2, m - 1]
    assert info[1]["c"] == m // 2 and info[2] == dict(k=m - 1, m=m, c=1, invert=True)
    if m > 2048:                                                # pieces of the last wave step are chosen
        assert all(set(want[s * 3 + 2]) & set(units[2][1][2048:]) for s in range(3))


def test_units_of_unequal_size_in_one_launch(ctx):
    """the launch's table is the largest unit's; the small units beside it use its first words"""
    r = random.Random(77)
    units = [UC.unit_of(r, 3, 1), UC.unit_of(r, 5000, 1700), UC.unit_of(r, 40, 39), ([(1, 2)], [(5, 9)]), UC.unit_of(r, 2100, 2000), UC.unit_of(r, 64, 32)]
    check_units(ctx, units, 2 ** 32 - 2, 0, 4)                  # (the unit streams' seeds wrap)


def test_segments_that_are_not_members(ctx):
    """segments that span pieces, touch borders or lie outside: k is the hit pieces, the sample whole pieces of W"""
    r = random.Random(5)
    units = []
    for _ in range(30):
        ws = UC.pieces(r, r.randint(1, 40), start=r.randint(0, 9))
        top = ws[-1][1] + 10
        segs = CIRC.rand_norm(r, r.randint(1, 12), top, r.choice([1, 4, 30]))
        units.append((segs, ws))
    units.append(([(1000, 1010)], UC.pieces(r, 5)))             # beyond the universe
    units.append(([(4, 6), (9, 10)], [(0, 4), (6, 9), (10, 12)]))          # in the gaps, touching the pieces on both sides
    info = []
    want = check_units(ctx, units, 21, 0, 5, info)
    assert any(st["k"] == 0 for st in info) and any(st["invert"] for st in info) and any(st["k"] > len(u[0]) for st, u in zip(info, units))
    for i, lst in enumerate(want):
        assert len(lst) == info[i]["k"] and set(lst) <= set(units[i % len(units)][1])


# ------------------------------------------------------------------------------------------------ whole problems
def test_split_sample_range(ctx):
    """two consecutive batches, the second with sample_begin > 0, give the lists of one batch"""
    r = random.Random(13)
    flat = UC.units_flat([UC.unit_of(r, m, k) for m, k in ((50, 10), (7, 4), (300, 290), (2500, 900), (1, 1))])
    whole, _ = device_units(ctx, flat, 99, 0, 13)
    first, _ = device_units(ctx, flat, 99, 0, 5)
    second, _ = device_units(ctx, flat, 99, 5, 13)
    assert first + second == whole
    assert whole == M.model_units(flat, 99, 0, 13)[0]


def test_isochore_units(ctx):
    """isochore keys with merge_contigs: one draw per (contig, isochore) unit; the contig lists are the units' lists one
    after the other, merge(0)d"""
    flat = UC.isochore_problem()
    assert int(flat["merge_contigs"]) == 1 and int(flat["n_units"]) == 7 and int(flat["n_contigs"]) == 3
    S = 9
    info = []
    want_units, ndraws = M.model_units(flat, 31, 0, S, info)
    assert sorted({st["k"] == 0 for st in info}) == [False, True] and any(st["k"] == st["m"] for st in info)
    want, want_off = CIRC.as_arrays(CIRC.contig_lists(flat, want_units, S))
    P = _lib.Problem(ctx, flat)
    try:
        got_units, got_unit_off = P.sample(31, 0, S, unit_level=True)
        assert P.last_stats["n_draws"] == ndraws
        got, got_off = P.sample(31, 0, S)
    finally:
        P.close()
    assert as_lists(got_units, got_unit_off) == want_units
    assert got_off.tolist() == want_off.tolist() and got.tolist() == want.tolist()
    assert len(want) < sum(len(x) for x in want_units)          # (touching pieces of two units, united in the contig list)


N_GRID = 66000                                                  # as tests/test_sampler_grid_z_gpu.py reaches blockIdx.z


def test_more_units_than_a_grid_dimension(ctx):
    """66 000 active units, 1 sample: a universe of two pieces per unit, one of them the segment (every fourth unit: both).
    Every unit's coordinates are its own, so a list written for the wrong unit cannot pass"""
    units = [(([(10 * u, 10 * u + 3)] if u % 2 else [(10 * u + 5, 10 * u + 9)]) if u % 4 else [(10 * u, 10 * u + 3), (10 * u + 5, 10 * u + 9)],
              [(10 * u, 10 * u + 3), (10 * u + 5, 10 * u + 9)]) for u in range(N_GRID)]
    flat = UC.units_flat(units)
    assert int((flat["unit_contig"] >= 0).sum()) == N_GRID > 65535
    got, st = device_units(ctx, flat, 7, 0, 1)
    assert len(got) == N_GRID
    picked = sorted({0, 32767, 32768, 65535, 65536, N_GRID - 1} | set(range(0, N_GRID, 33)))
    both = 0
    for u in picked:
        want = M.sample(O.RandomState((7 + u) & 0xFFFFFFFF), *units[u])
        assert got[u] == want, (u, got[u], want)
        both += want != units[u][0]
    assert both > 300                                           # (the draw moved the piece in a good part of them)
    for u, g in enumerate(got):
        assert len(g) == (1 if u % 4 else 2) and set(g) <= set(units[u][1]), (u, g)


# ------------------------------------------------------------------------------------------------ run()
def oracle_counts(flat, unit_lists, counters, S):
    """the oracle's counters over the contig lists of the (sample, unit) lists: [counter][track, sample]"""
    nc, nt = int(flat["n_contigs"]), int(flat["n_tracks"])
    lists = CIRC.contig_lists(flat, unit_lists, S)
    annos, off = O.aslist(flat["annos"]), flat["anno_off"]
    out = [np.zeros((nt, S), dtype=np.int64) for _ in counters]
    for k, name in enumerate(counters):
        for t in range(nt):
            for s in range(S):
                out[k][t, s] = sum(int(O.counter(name, lists[s * nc + c], annos[off[t * nc + c]:off[t * nc + c + 1]], int(flat["cws_nseg"][c])))
                                   for c in range(nc))
    return out


def test_run_counts(ctx, monkeypatch):
    """gat_amd.run(sampler=SamplerUniverse()) on a peak-set problem: every result's samples are the oracle's counters over the
    model's lists; the same run with null_round_size gives the same rows"""
    import null_fold_model as NF
    cfg = UC.peak_config()
    segments, annotations, workspace, _ = synthetic.as_collections(cfg)
    flats = []
    init = _lib.Problem.__init__

    def recording(self, c, flat, *args, **kwargs):
        flats.append(flat)
        return init(self, c, flat, *args, **kwargs)
    monkeypatch.setattr(_lib.Problem, "__init__", recording)
    S = 40

    def run(**kwargs):
        return gat_amd.run(segments, annotations, workspace, gat_amd.SamplerUniverse(), [gat_amd.COUNTERS[c]() for c in COUNTERS],
                           gat_amd.UnconditionalWorkspace(), num_samples=S, random_seed=31, **kwargs)
    results = run()
    assert len(flats) == 1 and int(flats[0]["sampler"]) == UC.UNIVERSE
    units = flats[0]                                            # (the units as run() laid them out)
    names = list(units["contig_names"])
    tracks = [t for t, _ in cfg["annotations"]]
    per = [[a.get(c, np.zeros(0, dtype=O.SEG)) for c in names] for _, a in cfg["annotations"]]
    flat = dict(units, n_tracks=len(tracks), annos=np.concatenate([x for t in per for x in t]),
                anno_off=np.concatenate([[0], np.cumsum([len(x) for t in per for x in t])]).astype(np.int64))
    info = []
    want_lists, _ = M.model_units(flat, 31, 0, S, info)
    assert [st["k"] for st in info[:3]] == [len(cfg["segments"][c]) for c in names] and [st["m"] for st in info[:3]] == [70, 55, 40]
    want = oracle_counts(flat, want_lists, COUNTERS, S)
    assert len(results) == len(tracks) * len(COUNTERS)
    for r in results:
        k, t = COUNTERS.index(r.counter), tracks.index(r.annotation)
        assert [int(v) for v in r.samples.tolist()] == want[k][t].tolist(), (r.counter, r.annotation)
        assert len(set(want[k][t].tolist())) > 3                # (the null is not one constant row)
    deep = run(null_round_size=7)
    assert len(deep) == len(results)
    for p, d in zip(results, deep):
        assert (p.track, p.annotation, p.counter, p.observed) == (d.track, d.annotation, d.counter, d.observed)
        assert d.null_words == NF.row_words([int(v) for v in p.samples.tolist()], p.observed), (d.counter, d.annotation)
        assert (d.nsamples, d.expected, d.pvalue, d.fold) == (S, p.expected, p.pvalue, p.fold)
        assert str(d).split("\t")[7:] == str(p).split("\t")[7:]


@pytest.mark.parametrize("method", ["minp", "efdr"])
def test_gat_run_script_prints_the_table(tmp_path, method):
    """scripts/gat-run.py --workspace=universe.bed --sampler=universe prints the usual table, with the joint-null q-values"""
    cfg = UC.peak_config()
    for name, per in (("s.bed", cfg["segments"]), ("universe.bed", cfg["workspace"])):
        (tmp_path / name).write_text("".join("%s\t%d\t%d\n" % (c, s, e) for c, a in per.items() for s, e in O.aslist(a)))
    (tmp_path / "a.bed").write_text("".join("track name=%s\n" % t + "".join("%s\t%d\t%d\n" % (c, s, e) for c, a in per.items() for s, e in O.aslist(a))
                                            for t, per in cfg["annotations"]))
    spec = importlib.util.spec_from_file_location("gat_run_cli_universe", os.path.join(ROOT, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "result.tsv"
    assert mod.main(["gat-run.py", "--segments=%s" % (tmp_path / "s.bed"), "--annotations=%s" % (tmp_path / "a.bed"),
                     "--workspace=%s" % (tmp_path / "universe.bed"), "--sampler=universe", "--num-samples=50", "--random-seed=4",
                     "--qvalue-method=%s" % method, "--stdout=%s" % out, "--log=%s" % (tmp_path / "log")]) == 0
    lines = [l for l in open(str(out)).read().splitlines() if l and not l.startswith("#")]
    assert lines[0].split("\t")[:4] == ["track", "annotation", "observed", "expected"]
    assert sorted(l.split("\t")[1] for l in lines[1:]) == ["t0", "t1", "t2"]


# ------------------------------------------------------------------------------------------------ a list consumer
def test_coverage_script_per_base(tmp_path):
    """gat-coverage --sampler=universe --bin-size=1 on a universe of seven pieces, three of them the segments: the model's
    per-base counts"""
    ws = [(10, 14), (16, 20), (20, 23), (30, 31), (35, 44), (50, 52), (55, 62)]
    segs = [(10, 14), (20, 23), (35, 44)]
    (tmp_path / "s.bed").write_text("".join("chr1\t%d\t%d\n" % x for x in segs))
    (tmp_path / "w.bed").write_text("".join("chr1\t%d\t%d\n" % x for x in ws))
    spec = importlib.util.spec_from_file_location("gat_coverage_cli_universe", os.path.join(ROOT, "scripts", "gat-coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "coverage.tsv"
    S = 25
    assert mod.main(["gat-coverage.py", "--stdout=%s" % out, "--segments=%s" % (tmp_path / "s.bed"), "--workspace=%s" % (tmp_path / "w.bed"),
                     "--num-samples=%d" % S, "--random-seed=9", "--bin-size=1", "--sampler=universe", "--verbose=0"]) == 0
    lines = open(str(out)).read().splitlines()
    assert not [l for l in lines[1:] if l.startswith("#")]                     # (nothing sampled beyond the last bin)
    rows = {int(f[2]): [int(x) for x in f[4:9]] for f in (l.split("\t") for l in lines[1:])}
    n_bins = 62
    bases, starts, ends = (np.zeros(n_bins, dtype=np.int64) for _ in range(3))
    seen = set()
    for s in range(S):                                                         # one unit: sample s draws from seed 9 + s
        lst = M.sample(O.RandomState(9 + s), segs, ws)
        assert len(lst) == 3 and set(lst) <= set(ws)
        seen.add(tuple(lst))
        b, a, e, outside = coverage_model.coverage_naive(lst, 1, n_bins)
        assert outside == 0
        bases, starts, ends = bases + b, starts + a, ends + e
    assert len(seen) > 8
    in_ws = {x for a, b in ws for x in range(a, b)}
    assert set(rows) == in_ws
    for x in sorted(in_ws):
        assert rows[x] == [1, int(any(a <= x < b for a, b in segs)), bases[x], starts[x], ends[x]], x


def test_problem_sample_returns_k_members(ctx):
    """Problem.sample: exactly k intervals per unit, every one a piece of W"""
    r = random.Random(8)
    units = [UC.unit_of(r, m, k) for m, k in ((12, 5), (1, 1), (200, 199), (33, 1), (640, 320))]
    flat = UC.units_flat(units)
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(17, 0, 6)                            # (one contig per unit: the contig lists are the units')
    finally:
        P.close()
    lists = as_lists(seg, off)
    assert len(lists) == 6 * len(units)
    for i, lst in enumerate(lists):
        segs, ws = units[i % len(units)]
        assert len(lst) == len(segs) and lst == sorted(lst) and len(set(lst)) == len(lst) and set(lst) <= set(ws)


def test_sampler_class(ctx):
    """SamplerUniverse.sample: numpy's seed convention, an isNormalized result, an empty list without a hit piece"""
    def slist(pairs):
        s = gat_amd.SegmentList(array=UC.seg_array(pairs))
        s.isNormalized = 1
        return s
    segs, ws = UC.unit_of(random.Random(3), 30, 7)
    s = gat_amd.SamplerUniverse()
    for seed in (0, 5, 2 ** 32 - 1):
        got = s.sample(slist(segs), slist(ws), seed=seed)
        assert got.isNormalized and [tuple(int(v) for v in x) for x in got] == M.sample(O.RandomState(seed), segs, ws)
    np.random.seed(3)
    seed = int(np.random.randint(0, 2 ** 32))
    np.random.seed(3)
    got = s.sample(slist(segs), slist(ws))
    assert [tuple(int(v) for v in x) for x in got] == M.sample(O.RandomState(seed), segs, ws)
    assert len(s.sample(slist([(ws[-1][1] + 3, ws[-1][1] + 8)]), slist(ws), seed=1)) == 0
    assert len(s.sample(slist([]), slist(ws), seed=1)) == 0 and len(s.sample(slist(segs), slist([]), seed=1)) == 0


def test_serial_mode_refused(ctx):
    flat = UC.units_flat([UC.unit_of(random.Random(4), 10, 3)])
    P = _lib.Problem(ctx, flat)
    try:
        state = np.zeros(_lib.MT_STATE_WORDS, dtype=np.uint32)
        state[-1] = 624
        with pytest.raises(Exception, match="SamplerUniverse runs on the per-unit streams only"):
            P.sample_and_count_serial(COUNTERS, state, 4)
    finally:
        P.close()


# ------------------------------------------------------------------------------------------------ the refusal
MOST = (160 * 1024 - 2560) // 4 // 64 * 2048                   # the generator's 2 560 bytes, whole wave steps of 64 words


def one_unit_of(m, segs):
    """a universe of m pieces [4 i, 4 i + 2), built without a Python loop"""
    ws = np.zeros(m, dtype=O.SEG)
    ws["start"] = np.arange(m, dtype=np.uint32) * 4
    ws["end"] = ws["start"] + 2
    return dict(n_units=1, segs=UC.seg_array(segs), seg_off=np.array([0, len(segs)], np.int64), ws=ws, ws_off=np.array([0, m], np.int64),
                unit_contig=np.array([0], np.int32), n_contigs=1, merge_contigs=0, n_tracks=0, annos=np.zeros(0, dtype=O.SEG),
                anno_off=np.zeros(1, np.int64), cws_nseg=np.array([m], np.int64), sampler=UC.UNIVERSE)


def test_oversized_unit_is_refused(ctx):
    """a unit of one piece more than the mark table in LDS takes: gat_problem_create's GAT_ERR_ARG as the Python error with
    the library's message.  No kernel is launched"""
    m = MOST + 1
    with pytest.raises(ValueError, match="unit 0: SamplerUniverse: %d workspace pieces, the mark table in LDS takes at most %d" % (m, MOST)):
        _lib.Problem(ctx, one_unit_of(m, [(0, 2)]))


def test_largest_unit_runs(ctx):
    """the largest unit that is not refused -- the launch takes all of the LDS limit --, two pieces hit, the last among them"""
    m = MOST
    flat = one_unit_of(m, [(0, 2), (4 * (m - 1), 4 * (m - 1) + 2)])
    got, st = device_units(ctx, flat, 6, 0, 3)
    ndraws = 0
    for s in range(3):
        rng = O.RandomState(6 + s)
        marked = sorted(M.floyd(lambda j: rng.randint(0, j + 1), m, 2))
        ndraws += rng.ndraws
        assert got[s] == [(4 * h, 4 * h + 2) for h in marked], (s, got[s], marked)
    assert st["n_draws"] == ndraws and len({tuple(g) for g in got}) == 3
