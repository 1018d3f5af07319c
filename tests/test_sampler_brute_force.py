"""GPU: SamplerBruteForce (gat/Engine.pyx:746-871) through the C ABI against tests/brute_force_model.py -- the reference's
loop restated on the oracle's RandomState, pinned to the reference's own output by tests/test_brute_force_model.py.
Bit-exact: the sampled (sample, unit) lists, the statistics and the count matrices."""
import random

import numpy as np
import pytest

import brute_force_model as M
import sampler_edges as E
from gat_amd import _lib, problem, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu
BRUTE = 5                               # GAT_SAMPLER_BRUTE_FORCE
LDS_LIST = 256                          # accepted segments k_brute_force keeps in LDS (gat_brute_force.h: kBruteLdsCap)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _flat(units, bucket_size=1, ntries_inner=0, ntries_outer=0):
    flat = E.units_flat(units, BRUTE)
    flat.update(bucket_size=bucket_size, nbuckets=100000, brute_ntries_inner=ntries_inner, brute_ntries_outer=ntries_outer)
    return flat


def _units_of(flat):
    segs, ws = O.aslist(flat["segs"]), O.aslist(flat["ws"])
    so, wo = flat["seg_off"], flat["ws_off"]
    return [(segs[so[u]:so[u + 1]], ws[wo[u]:wo[u + 1]]) for u in range(int(flat["n_units"]))]


def _model(flat, seed, s0, s1):
    st = {}
    kw = dict(bucket_size=int(flat.get("bucket_size", 1)))
    if flat.get("brute_ntries_inner"):
        kw.update(ntries_inner=flat["brute_ntries_inner"], ntries_outer=flat["brute_ntries_outer"])
    return M.model_units(_units_of(flat), seed, s0, s1, stats=st, **kw), st


def _check_stats(st, mst):
    assert st["n_draws"] == mst["n_draws"] and st["n_restarts"] == mst["restarts"] and st["n_unconverged"] == 0
    assert st["n_placed"] == mst["placed"] and st["n_unsuccessful"] == mst["tries"]


def _random_units(r, n):
    """3 to 12 segments of 1..6 bases in 1 to 4 workspace pieces of 300..600 bases"""
    units = []
    for _ in range(n):
        ws, x = [], r.randint(0, 50)
        for _ in range(r.randint(1, 4)):
            ln = r.randint(300, 600)
            ws.append((x, x + ln))
            x += ln + r.choice([0, 1, 3, 40])          # (0: adjacent pieces; 1, 3: closer together than a length)
        segs = [(s, s + r.randint(1, 6)) for s in sorted(r.sample(range(ws[0][0], ws[-1][1], 8), r.randint(3, 12)))]
        units.append((segs, ws))
    return units


def test_random_units_vs_model(ctx):
    """8 units x 16 samples; some (sample, unit) restarts, every one converges."""
    flat = _flat(_random_units(random.Random(11), 8))
    want, mst = _model(flat, 4321, 0, 16)
    assert mst["restarts"] > 0 and mst["unconverged"] == 0 and mst["tries"] > 0
    got, st = E.device_units(ctx, flat, 4321, 0, 16)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    _check_stats(st, mst)


def _one_piece_unit(r, n, span):
    """n segments of 1..12 bases in one piece, a segment of one base among them (the last base can always be placed)"""
    return ([(1, 2)] + [(s, s + r.randint(1, 12)) for s in sorted(r.sample(range(10, span, 16), n - 1))], [(0, span + 100)])


@pytest.mark.parametrize("n,lo,hi", [(70, 60, 70), (130, 120, 130), (300, LDS_LIST + 1, 400)])
def test_list_length_edges(ctx, n, lo, hi):
    """accepted lists across one wave width, two wave widths, and the LDS list's capacity into the slab"""
    r = random.Random(n)
    flat = _flat([_one_piece_unit(r, n, 40 * n)])
    want, mst = _model(flat, 99, 0, 8)
    assert mst["unconverged"] == 0 and any(lo <= len(w) <= hi for w in want), sorted(len(w) for w in want)
    got, st = E.device_units(ctx, flat, 99, 0, 8)
    assert got == want
    _check_stats(st, mst)


def test_slab_overflow_retry(ctx):
    """GAT_TEST_SMALL_CAPS: the regions start at their smallest -- 320 slots for the unit of 300 segments (half of twice
    its segments + 8, in whole 64s) --, a sample whose list is longer overflows, the slab is laid out again and the batch
    repeated from the same seeds; what it counts, it counts once.  One sample per call: its lists fit the 1 024 segments
    Problem.sample asks for first, so the call is not made a second time (whose statistics would show no retry)."""
    r = random.Random(5)
    flat = _flat(_random_units(r, 6) + [_one_piece_unit(r, 300, 12000)])
    n = int(flat["n_units"])
    lists, _ = _model(flat, 3, 0, 6)
    s = max(range(6), key=lambda i: len(lists[i * n + n - 1]))
    assert len(lists[s * n + n - 1]) > 320 and sum(len(l) for l in lists[s * n:(s + 1) * n]) <= 1024
    ctx.options["GAT_TEST_SMALL_CAPS"] = "1"
    try:
        got, st = E.device_units(ctx, flat, 3, s, s + 1)
    finally:
        ctx.options.pop("GAT_TEST_SMALL_CAPS", None)
    want, mst = _model(flat, 3, s, s + 1)
    assert mst["unconverged"] == 0
    assert got == want
    assert st["n_retried"] > 0
    _check_stats(st, mst)


def test_split_sample_ranges(ctx):
    flat = _flat(_random_units(random.Random(12), 8))
    whole, _ = E.device_units(ctx, flat, 77, 0, 16)
    a, _ = E.device_units(ctx, flat, 77, 0, 5)
    b, _ = E.device_units(ctx, flat, 77, 5, 16)
    assert a + b == whole
    assert whole == _model(flat, 77, 0, 16)[0]


def _genome_flat():
    """synthetic.small_genome with isochores, every fourth segment, cut to 1 or 2 bases (so that the units converge)"""
    _, cfg = synthetic.small_genome()
    segs = cfg["segments"]
    for c in segs:
        a = segs[c][::4].copy()
        a["end"] = a["start"] + 1 + (a["end"] - a["start"] - 1) % 2
        segs[c] = a
    flat = problem.flatten_arrays(segs, cfg["annotations"], cfg["workspace"], cfg["isochores"], bucket_size=1)
    flat["sampler"] = BRUTE
    return flat


def test_isochore_problem_counts(ctx):
    """isochore units feeding k_contig: the (sample, unit) lists, the contig lists and all six counters"""
    flat = _genome_flat()
    assert int(flat["merge_contigs"]) == 1
    S = 6
    want_lists, mst = _model(flat, 21, 0, S)
    assert mst["unconverged"] == 0
    got, st = E.device_units(ctx, flat, 21, 0, S)
    assert got == want_lists
    _check_stats(st, mst)
    want = E.model_counts(flat, want_lists, E.ALL_COUNTERS, S)
    n, nc = int(flat["n_units"]), int(flat["n_contigs"])
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(21, 0, S)
        counts = P.sample_and_count(E.ALL_COUNTERS, 21, 0, S)
    finally:
        P.close()
    contig_lists = E.as_lists(seg, off)
    for s in range(S):
        for c in range(nc):
            units = [want_lists[s * n + u] for u in range(n) if int(flat["unit_contig"][u]) == c]
            merged = O.aslist(O.merge(sorted(x for l in units for x in l), 0)) if any(units) else []
            assert contig_lists[s * nc + c] == [tuple(x) for x in merged], (s, c)
    for k, name in enumerate(E.ALL_COUNTERS):
        assert np.array_equal(counts[k], want[k]), name


@pytest.mark.parametrize("bucket_size", [0, 7])
def test_bucket_sizes(ctx, bucket_size):
    """bucket_size 0 (automatic) and 7 (a second draw inside the bucket)"""
    r = random.Random(40 + bucket_size)
    units = [([(s, s + r.randint(1, 20)) for s in sorted(r.sample(range(0, 3000, 32), r.randint(5, 20)))] + [(3100, 3101)],
              [(0, 1500), (1510, 3200)]) for _ in range(6)]
    flat = _flat(units, bucket_size=bucket_size)
    seed = {0: 8, 7: 12}[bucket_size]         # (bucket_size 7 draws lengths of 7..27 only: a seed under which all 48 converge)
    want, mst = _model(flat, seed, 0, 8)
    assert mst["unconverged"] == 0, mst
    got, st = E.device_units(ctx, flat, seed, 0, 8)
    assert got == want
    _check_stats(st, mst)


DENSE = ([(100 + 10 * i, 100 + 10 * i + 3 + i % 5) for i in range(30)], [(90, 390)])


def test_non_convergence(ctx):
    """ntries_inner=3, ntries_outer=2 on the dense unit: a sample range in which some (sample, unit) does not converge
    raises the reference's ValueError and counts it; a range in which all converge matches the model.  (A status path,
    not a fault.)"""
    flat = _flat([DENSE], ntries_inner=3, ntries_outer=2)
    lists, _ = _model(flat, 5, 0, 8)
    good = [l is not None for l in lists].index(True)          # (one sample in a hundred converges: sample 2 of this seed)
    bad = [l is None for l in lists[good:]].index(True) + good
    assert 0 < good < bad
    P = _lib.Problem(ctx, flat)
    # (the same unit with one annotation track of one segment: the counting path)
    Pc = _lib.Problem(ctx, dict(flat, n_tracks=1, annos=np.array([(100, 200)], dtype=O.SEG), anno_off=np.array([0, 1], np.int64)))
    dev = ctx.alloc(8 * (bad + 1 - good))
    try:
        with pytest.raises(ValueError, match="did not converge"):
            P.sample(5, good, bad + 1, unit_level=True)
        assert P.last_stats["n_unconverged"] == sum(l is None for l in lists[good:bad + 1]) > 0
        msg = _lib.lib().gat_last_error(ctx._h).decode()
        assert "sample %d, unit 0" % bad in msg, msg
        # ... on the counting path as well (what run() takes, sharded or not); no counts come back
        with pytest.raises(ValueError, match="did not converge"):
            Pc.sample_and_count(["nucleotide-overlap"], 5, bad, bad + 1)
        assert Pc.last_stats["n_unconverged"] == 1
        Pc.enqueue(["nucleotide-overlap"], 5, good, bad + 1, dev)
        with pytest.raises(ValueError, match="did not converge"):
            Pc.wait()
        assert Pc.last_stats["n_unconverged"] > 0
        got = Pc.sample_and_count(["nucleotide-overlap"], 5, good, good + 1)       # (the problem goes on working)
        want_ov = sum(min(e, 200) - max(s, 100) for s, e in lists[good] if min(e, 200) > max(s, 100))
        assert got[0].shape == (1, 1) and int(got[0][0, 0]) == want_ov
        seg, off = P.sample(5, good, good + 1, unit_level=True)
        want, mst = _model(flat, 5, good, good + 1)
        assert E.as_lists(seg, off) == want
        _check_stats(P.last_stats, mst)
    finally:
        ctx.free(dev)
        P.close()
        Pc.close()


def test_negative_tries_refused(ctx):
    for kw in (dict(ntries_inner=-1), dict(ntries_outer=-1)):
        with pytest.raises(ValueError):
            _lib.Problem(ctx, _flat([DENSE], **kw))


def test_no_reference_stream(ctx):
    P = _lib.Problem(ctx, _flat([DENSE]))
    try:
        state = np.zeros(_lib.MT_STATE_WORDS, dtype=np.uint32)
        state[-1] = 624
        with pytest.raises(Exception):
            P.sample_and_count_serial(["nucleotide-overlap"], state, 4)
    finally:
        P.close()


def test_kats_exact_through_the_class():
    """the reference's own single-unit known answers (tests/golden/brute_force/kat.json) through
    gat_amd.SamplerBruteForce.sample: every hand-made shape the library takes and the first sixty random ones -- the list, or
    the reference's ValueError."""
    import gat_amd
    cases = M.load_kats()
    picked = [c for c in cases if c["kind"] == "fixed" and max(e for _, e in c["segments"]) < 2 ** 31]
    picked += [c for c in cases if c["kind"] == "random"][:60]
    raised = 0
    for i, c in enumerate(picked):
        sampler = gat_amd.SamplerBruteForce(**c["params"])
        segs = gat_amd.SegmentList(iter=c["segments"], normalize=True)
        ws = gat_amd.SegmentList(iter=c["workspace"], normalize=True)
        if c["error"]:
            with pytest.raises(ValueError):
                sampler.sample(segs, ws, seed=c["seed"])
            raised += 1
        else:
            assert sampler.sample(segs, ws, seed=c["seed"]).asList() == c["sample"], i
    assert raised > 0 and len(picked) - raised >= 60


def test_cli_tables_byte_equal(tmp_path):
    """scripts/gat-run.py -m brute-force prints the reference's table (per-unit stream patch) byte for byte."""
    import importlib.util
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("gat_run_cli_brute", os.path.join(here, "..", "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cli_in, gold = os.path.join(here, "golden", "cli"), os.path.join(here, "golden", "brute_force", "cli")
    cases = json.load(open(os.path.join(gold, "cases.json")))
    assert set(cases) == {"plain", "isochores", "segment_tracks", "conditional"}
    for name, extra in cases.items():
        extra = [x.replace("--isochores=", "--isochores=%s%s" % (cli_in, os.sep)).replace("--sampler=brute-force", "-m brute-force")
                 for x in extra]
        extra = [y for x in extra for y in x.split(" ")]
        out = str(tmp_path / ("%s.tsv" % name))
        argv = ["gat-run.py", "--segments=%s" % os.path.join(gold, "segments.bed"),
                "--annotations=%s" % os.path.join(cli_in, "annotations.bed"),
                "--workspace=%s" % os.path.join(cli_in, "workspace.bed"), "--stdout=%s" % out,
                "--log=%s" % str(tmp_path / "log")] + extra
        assert mod.main(argv) == 0
        got = [l for l in open(out) if not l.startswith("#")]
        want = [l for l in open(os.path.join(gold, "expected_%s.tsv" % name))]
        assert got == want, name
