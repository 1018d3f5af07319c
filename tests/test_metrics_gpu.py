"""GPU: k_metrics.  gat_list_metrics against the model (tests/metrics_model.py) on hand-made and fuzzed geometry, gat_sample_metrics
against the model applied to Problem.sample of the SAME problem, seed and sample range, and scripts/gat-run.py against the
reference's own table and side files (tests/golden/metrics/cli).  Every comparison is exact: integers, or the bytes of a file."""
import json
import os
import random

import numpy as np
import pytest

import coverage_cases as CC
import metrics_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
GOLD = os.path.join(ROOT, "tests", "golden", "metrics", "cli")
TOP = 2 ** 31 - 1
LDS_PIECES = 64


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    c.options["GAT_METRICS_LDS_PIECES"] = str(LDS_PIECES)         # the tests' staging limit: 65 pieces and more end in global memory
    yield c
    c.close()


def seg_array(pairs):
    a = np.zeros(len(pairs), dtype=_lib.SEG)
    if len(pairs):
        a["start"], a["end"] = np.array(pairs, dtype=np.int64).T
    return a


def device_words(ctx, lists, workspaces):
    """lists[l][g] and workspaces[g] as lists of (start, end) -> int64 [n_lists, n_groups, 8] from gat_list_metrics"""
    n_lists, n_groups = len(lists), len(workspaces)
    flat = [lists[l][g] for l in range(n_lists) for g in range(n_groups)]
    list_off = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64)
    ws_off = np.concatenate([[0], np.cumsum([len(w) for w in workspaces])]).astype(np.int64)
    return _lib.list_metrics(ctx, seg_array([p for x in flat for p in x]), list_off, n_lists,
                             seg_array([p for w in workspaces for p in w]), ws_off, n_groups)


def check_lists(ctx, lists, workspaces, what=""):
    got = device_words(ctx, lists, workspaces)
    assert got.dtype == np.int64 and got.shape == (len(lists), len(workspaces), len(M.WORDS))
    for l in range(len(lists)):
        for g in range(len(workspaces)):
            want = M.words(lists[l][g], workspaces[g])
            assert got[l, g].tolist() == want, (what, l, g, got[l, g].tolist(), want)
    return got


def pieces(n, first=100, length=7, gap_every=3):
    """n pieces of `length` bases from `first` on; every gap_every-th neighbour adjacent, the others 5 bases apart"""
    out, pos = [], first
    for j in range(n):
        out.append((pos, pos + length))
        pos += length + (0 if j % gap_every == 0 else 5)
    return out


def fuzz_list(r, n, span):
    """n sorted, disjoint segments of 1..12 bases over about `span` bases, three in ten neighbours adjacent"""
    out, pos = [], r.randint(0, 20)
    for _ in range(n):
        ln = r.randint(1, 12)
        out.append((pos, pos + ln))
        pos += ln + (0 if r.random() < 0.3 else r.randint(1, max(2, span // n)))
    return out


# ---- 1. gat_list_metrics: hand-made geometry -------------------------------------------------------------------------------
WS3 = [(100, 200), (200, 300), (350, 400)]
GEOMETRY = [
    ("empty list", [], WS3),
    ("empty workspace", [(10, 20), (30, 40)], []),
    ("both empty", [], []),
    ("equal to a piece", [(200, 300)], WS3),
    ("e == piece.start", [(50, 100)], WS3),
    ("s == piece.end", [(300, 350)], WS3),
    ("between two pieces, touching both", [(300, 350)], [(100, 300), (350, 400)]),
    ("over two adjacent pieces", [(150, 250)], WS3),
    ("over two pieces with a gap", [(250, 380)], WS3),
    ("over all pieces", [(50, 500)], WS3),
    ("exactly all pieces", [(100, 400)], WS3),
    ("before the first piece", [(0, 10), (20, 99)], WS3),
    ("after the last piece", [(400, 410), (1000, 2000)], WS3),
    ("before, inside, after", [(0, 10), (90, 110), (120, 130), (190, 210), (299, 351), (399, 401), (500, 600)], WS3),
    ("top coordinates", [(TOP - 1000, TOP - 500), (TOP - 400, TOP)], [(TOP - 700, TOP - 450), (TOP - 450, TOP - 100), (TOP - 50, TOP)]),
    ("top, outside", [(TOP - 10, TOP)], [(0, 5)]),
    ("one base", [(5, 6)], [(5, 6)]),
    ("unsorted, overlapping", [(390, 420), (150, 250), (0, 10), (160, 170), (150, 250), (500, 600), (90, 360), (395, 396)], WS3),
    ("unsorted, the last toucher first", [(399, 401), (0, 10), (450, 460), (120, 130), (398, 500)], WS3),
]


def test_geometry_each_alone(ctx):
    for name, segs, ws in GEOMETRY:
        check_lists(ctx, [[segs]], [ws], name)


def test_geometry_in_one_call(ctx):
    """every list against every workspace: n_lists x n_groups lists in one launch, most of them not made for each other"""
    wss = [ws for _, _, ws in GEOMETRY]
    lists = [[segs for _ in wss] for _, segs, _ in GEOMETRY]
    got = check_lists(ctx, lists, wss, "all pairs")
    assert got[:, :, 2].sum() > 0 and got[:, :, 6].sum() > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_list_lengths(ctx, n):
    """a wave's stride over its list: lengths around one and four rounds of 64 lanes, sorted and shuffled"""
    r = random.Random(n)
    ws = [(0, 40)] + pieces(40, first=45, length=9)         # (a list's first segment starts below 21: it meets the first piece)
    segs = fuzz_list(r, n, 1500)
    assert len(segs) == n
    shuffled = list(segs)
    r.shuffle(shuffled)
    got = check_lists(ctx, [[segs], [shuffled]], [ws], n)
    assert got[0, 0].tolist() == got[1, 0].tolist() and got[0, 0, 2] > 0           # (no word depends on the order)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 4 * LDS_PIECES + 3])
def test_piece_counts(ctx, k):
    """groups of k pieces: up to GAT_METRICS_LDS_PIECES (64 here) the searches stay in LDS, beyond it they find a block of
    ceil(k / 64) pieces there and end in global memory"""
    r = random.Random(k)
    ws = pieces(k)
    top = ws[-1][1]
    segs = [(0, 50), (0, top + 10), (ws[0][0], ws[0][1]), (ws[-1][0], ws[-1][1]), (ws[-1][1], ws[-1][1] + 5), (ws[k // 2][0] + 1, ws[k // 2][1] + 3)]
    segs += [(s, s + r.randint(1, 40)) for s in (r.randint(0, top + 30) for _ in range(300))]
    segs += [(w[0], w[1]) for w in ws[::5]] + [(w[1], w[1] + 5) for w in ws[::7]] + [(w[0] - 3, w[0]) for w in ws[1::7]]
    got = check_lists(ctx, [[segs, sorted(segs)]], [ws, ws], k)
    assert got[0, 0].tolist() == got[0, 1].tolist() and got[0, 0, 2] > k


def test_staging_limit_changes_no_result(ctx, monkeypatch):
    r = random.Random(3)
    wss = [pieces(k, first=10 + k) for k in (1, 64, 65, 200, 1000)]
    lists = [[[(s, s + r.randint(1, 60)) for s in (r.randint(0, 14000) for _ in range(150))] for _ in wss] for _ in range(5)]
    want = check_lists(ctx, lists, wss)
    for limit in ("1", "7", "200", "2048", "100000000"):
        monkeypatch.setitem(ctx.options, "GAT_METRICS_LDS_PIECES", limit)
        assert np.array_equal(device_words(ctx, lists, wss), want), limit


def test_many_lists_and_groups(ctx):
    """more lists than a workgroup's run, more than one workgroup per group; empty lists and empty groups among them"""
    r = random.Random(11)
    wss = [pieces(r.choice([0, 1, 3, 70]), first=r.randint(0, 50)) for _ in range(7)]
    lists = [[fuzz_list(r, r.choice([0, 1, 5, 70]), 600) for _ in wss] for _ in range(150)]
    check_lists(ctx, lists, wss)


def test_list_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    segs, ws = seg_array([(1, 5), (7, 9)]), seg_array([(0, 4), (4, 8)])
    off, woff = np.array([0, 2], dtype=np.int64), np.array([0, 2], dtype=np.int64)
    out = np.full((1, 1, 8), -1, dtype=np.int64)

    def call(c=ctx._h, lists=segs, lo=off, n=1, w=ws, wo=woff, g=1, o=out):
        return L.gat_list_metrics(c, p(lists), p(lo), n, p(w), p(wo), g, p(o))

    assert call() == 0 and out[0, 0].tolist() == M.words([(1, 5), (7, 9)], [(0, 4), (4, 8)])
    for bad in (dict(c=None), dict(lo=None), dict(wo=None), dict(o=None), dict(n=-1), dict(g=-1), dict(lists=None), dict(w=None),
                dict(lo=np.array([2, 0], dtype=np.int64)), dict(wo=np.array([2, 0], dtype=np.int64)),
                dict(lists=seg_array([(5, 1), (7, 9)])), dict(w=seg_array([(0, 4), (3, 8)])), dict(w=seg_array([(4, 8), (0, 4)])),
                dict(w=seg_array([(0, 4), (6, 6)]))):
        assert call(**bad) == -6, bad
    assert b"not normalized" in L.gat_last_error(ctx._h)
    # nothing to measure: no launch, nothing written
    assert call(n=0, lo=np.array([0], dtype=np.int64)) == 0 and call(g=0, lo=np.array([0], dtype=np.int64), wo=np.array([0], dtype=np.int64)) == 0
    # segments of no bases are segments
    assert call(lists=seg_array([(2, 2), (9, 9)])) == 0 and out[0, 0].tolist() == M.words([(2, 2), (9, 9)], [(0, 4), (4, 8)])


# ---- 2. gat_sample_metrics ------------------------------------------------------------------------------------------------------
SEED, SAMPLES = 77, 12


def contig_pieces(flat):
    """per contig of the problem, in its order: the union of its units' workspaces (merged where the problem has isochore
    keys, as IntervalDictionary.fromIsochores does; else the unit's list as it is)"""
    per = [[] for _ in range(int(flat["n_contigs"]))]
    for u, c in enumerate(flat["unit_contig"]):
        if c >= 0:
            w = flat["ws"][flat["ws_off"][u]:flat["ws_off"][u + 1]]
            per[c] += list(zip(w["start"].tolist(), w["end"].tolist()))
    if int(flat["merge_contigs"]):
        for c, lst in enumerate(per):
            merged = []
            for s, e in sorted(lst):
                if merged and s <= merged[-1][1]:
                    merged[-1] = (merged[-1][0], max(merged[-1][1], e))
                else:
                    merged.append((s, e))
            per[c] = merged
    return per


def check_samples(P, flat, seed, s0, s1):
    per = contig_pieces(flat)
    ws_off = np.concatenate([[0], np.cumsum([len(w) for w in per])]).astype(np.int64)
    ws = seg_array([p for w in per for p in w])
    seg, off = P.sample(seed, s0, s1)
    got = P.sample_metrics(seed, s0, s1, ws, ws_off)
    C_ = P.n_contigs
    assert got.dtype == np.int64 and got.shape == (s1 - s0, C_, len(M.WORDS))
    for i in range(s1 - s0):
        for c in range(C_):
            a = seg[off[i * C_ + c]:off[i * C_ + c + 1]]
            want = M.words(list(zip(a["start"].tolist(), a["end"].tolist())), per[c])
            assert got[i, c].tolist() == want, (i, c, got[i, c].tolist(), want)
    return got, ws, ws_off


@pytest.mark.parametrize("name", sorted(CC.SIX))
def test_six_samplers(ctx, name):
    flat = CC.SIX[name]()
    P = _lib.Problem(ctx, flat)
    try:
        got, ws, ws_off = check_samples(P, flat, SEED, 0, SAMPLES)
        assert got[:, :, 0].sum() > 0 and got[:, :, 3].sum() > 0
        # the range cut in two, and again in batches of a few samples: the same words
        a, b = P.sample_metrics(SEED, 0, 5, ws, ws_off), P.sample_metrics(SEED, 5, SAMPLES, ws, ws_off)
        assert np.array_equal(np.concatenate([a, b]), got)
    finally:
        P.close()


def test_isochore_contig_with_several_units_and_many_batches(ctx, monkeypatch):
    flat = CC.genome_problem(CC.ANNOTATOR, True)
    units_per_contig = np.bincount(flat["unit_contig"][flat["unit_contig"] >= 0])
    assert flat["merge_contigs"] == 1 and units_per_contig.max() > 1
    P = _lib.Problem(ctx, flat)
    try:
        whole, ws, ws_off = check_samples(P, flat, 8, 0, 24)
        assert P.last_stats["n_batches"] == 1
    finally:
        P.close()
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")      # (a scratch budget of a few samples, for a problem made under it)
    P = _lib.Problem(ctx, flat)
    try:
        cut = P.sample_metrics(8, 0, 24, ws, ws_off)
        assert P.last_stats["n_batches"] > 3, P.last_stats["n_batches"]
        assert np.array_equal(cut, whole)
    finally:
        P.close()


def test_sample_arguments(ctx):
    L = _lib.lib()
    p = _lib._p
    flat = CC.unit_problem("annotator")
    P = _lib.Problem(ctx, flat)
    try:
        per = contig_pieces(flat)
        ws_off = np.concatenate([[0], np.cumsum([len(w) for w in per])]).astype(np.int64)
        ws = seg_array([q for w in per for q in w])
        out = np.full((2, P.n_contigs, 8), -1, dtype=np.int64)

        def call(c=ctx._h, prob=P._h, begin=0, end=2, w=ws, wo=ws_off, o=out):
            return L.gat_sample_metrics(c, prob, 5, begin, end, p(w), p(wo), p(o), None)

        assert call() == 0 and out.min() >= 0
        bad_ws = ws.copy()
        bad_ws["start"][1] = bad_ws["end"][1]
        down = ws_off.copy()
        down[1] = down[2] + 1
        for bad in (dict(c=None), dict(prob=None), dict(wo=None), dict(o=None), dict(begin=3, end=2), dict(w=bad_ws), dict(wo=down), dict(w=None)):
            assert call(**bad) == -6, bad
        keep = out.copy()
        assert call(begin=4, end=4) == 0 and np.array_equal(out, keep)        # an empty range writes nothing
        dev = ctx.alloc(8)
        try:
            P.enqueue(["nucleotide-overlap"], 5, 0, 2, dev)
            assert call() == -6 and b"in flight" in L.gat_last_error(ctx._h)
            P.wait()
        finally:
            ctx.free(dev)
        assert call() == 0 and np.array_equal(out, keep)
    finally:
        P.close()


def test_sampler_errors_pass_through(ctx):
    import brute_force_edges as BF
    case = [c for c in BF.fixed_units() if c["name"] == "sum_beyond_workspace"][0]
    flat = BF.units_flat(case["units"], **case["params"])
    P = _lib.Problem(ctx, flat)
    try:
        per = contig_pieces(flat)
        with pytest.raises(ValueError, match="did not converge"):
            P.sample_metrics(1, 0, 1, seg_array([q for w in per for q in w]), np.concatenate([[0], np.cumsum([len(w) for w in per])]))
        assert P.last_stats["n_unconverged"] == 1
    finally:
        P.close()


# ---- 3. the command line ------------------------------------------------------------------------------------------------------------
def run_cli(tmp_path, tag, extra):
    from test_metrics_host import base_argv, script
    d = tmp_path / tag
    d.mkdir()
    pat = str(d / "side.%s")
    assert script().main(base_argv(d, ["-P", pat] + extra)) == 0
    table = "".join(l for l in open(d / "table.tsv") if not l.startswith("#"))
    return table, pat, sorted(os.listdir(d))


@pytest.mark.parametrize("name", ["plain", "tracks", "isochores"])
def test_cli_reproduces_the_reference_files(tmp_path, name):
    """the reference's gat-run.py (per-unit streams; Stats.Summary's two integer divisions mended) wrote these bytes"""
    extra = json.load(open(os.path.join(GOLD, "cases.json")))[name]
    table, pat, _ = run_cli(tmp_path, "with", extra)
    assert table == open(os.path.join(GOLD, "expected_%s.tsv" % name)).read()
    sides = [s for s in ("segment_metrics", "sample_metrics") if "--output-stats=%s" % s in extra]
    assert sides
    for s in sides:
        assert open(pat % s).read() == open(os.path.join(GOLD, "expected_%s.%s" % (name, s))).read(), s
    # the table is the one of a run without the options
    plain, _, files = run_cli(tmp_path, "without", [x for x in extra if not x.startswith("--output-stats")])
    assert plain == table and files == ["log", "table.tsv"]


def test_cli_sample_metrics_with_isochores(ctx, tmp_path):
    """not in the reference's reach (it looks contigs up in an isochore-keyed workspace and reports every sample as wholly
    outside): a contig's samples against the contig's workspace.  The file is the model's sums over Problem.sample of the same
    inputs, seed and range -- the samples the table was made from -- in metrics.write_rows' text (which the goldens pin)."""
    import io
    import gat_amd
    from gat_amd import coverage, metrics
    from gat_amd import io as IO
    from test_metrics_host import base_argv
    extra = ["--num-samples=6", "--random-seed=53", "--isochores=isochores.bed", "--output-stats=sample_metrics"]
    _, pat, _ = run_cli(tmp_path, "iso", extra)
    text = open(pat % "sample_metrics").read()
    opts, _ = gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS).parse_args(base_argv(tmp_path, extra[:3])[1:])
    segments, annotations, workspaces, isochores = IO.buildSegments(opts)
    workspace = IO.applyIsochores(segments, annotations, workspaces, opts, isochores)
    flat, _, _ = coverage.flatten(segments["merged"], workspace, coverage.make_sampler(opts))
    assert flat["merge_contigs"] == 1 and flat["n_units"] > flat["n_contigs"]
    ws, ws_off, size = metrics.contig_workspace(workspace, flat["contig_names"])
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(53, 0, 6)
    finally:
        P.close()
    nc = int(flat["n_contigs"])
    words = np.array([[M.words_of_array(seg[off[i * nc + c]:off[i * nc + c + 1]], ws[ws_off[c]:ws_off[c + 1]]) for c in range(nc)]
                      for i in range(6)], dtype=np.int64)
    want = io.StringIO()
    want.write(metrics.HEADER)
    metrics.write_rows(want, "merged", [str(i) for i in range(6)], words, size)
    assert text == want.getvalue()
    assert len(text.splitlines()) == 1 + 6 * 10 and words[:, :, 3].sum() > 0          # (not "wholly outside")


def test_cli_sample_metrics_circular(ctx, tmp_path):
    """--sampler=circular (not in the reference either): the file is the model's sums over Problem.sample of the same inputs,
    seed and range -- the lists a rotation cuts at the workspace's borders, a contig's pieces counted one by one"""
    import io
    import gat_amd
    from gat_amd import coverage, metrics
    from gat_amd import io as IO
    from test_metrics_host import base_argv
    extra = ["--num-samples=6", "--random-seed=53", "--sampler=circular", "--output-stats=sample_metrics"]
    _, pat, _ = run_cli(tmp_path, "circular", extra)
    text = open(pat % "sample_metrics").read()
    opts, _ = gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS).parse_args(base_argv(tmp_path, extra[:3])[1:])
    segments, annotations, workspaces, isochores = IO.buildSegments(opts)
    workspace = IO.applyIsochores(segments, annotations, workspaces, opts, isochores)
    flat, _, _ = coverage.flatten(segments["merged"], workspace, coverage.make_sampler(opts))
    assert flat["sampler"] == 6 and flat["merge_contigs"] == 0 and flat["n_units"] == flat["n_contigs"]
    ws, ws_off, size = metrics.contig_workspace(workspace, flat["contig_names"])
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(53, 0, 6)
    finally:
        P.close()
    nc = int(flat["n_contigs"])
    words = np.array([[M.words_of_array(seg[off[i * nc + c]:off[i * nc + c + 1]], ws[ws_off[c]:ws_off[c + 1]]) for c in range(nc)]
                      for i in range(6)], dtype=np.int64)
    want = io.StringIO()
    want.write(metrics.HEADER)
    metrics.write_rows(want, "merged", [str(i) for i in range(6)], words, size)
    assert text == want.getvalue()
    assert len(text.splitlines()) == 1 + 6 * 10 and words[:, :, 3].sum() > 0
    assert len({words[i].tobytes() for i in range(6)}) > 1                       # (the samples differ: a rotation each)


def test_cli_all_writes_the_files_it_wrote_before(tmp_path):
    """--output-stats=all: the collection summaries, neither of the two metrics files"""
    _, _, files = run_cli(tmp_path, "all", ["--num-samples=3", "--random-seed=1", "--output-stats=all"])
    sides = [f[len("side."):] for f in files if f.startswith("side.")]
    assert sides and all(s.startswith("stats_") or s.startswith("overlap_") for s in sides), sides
