"""GPU: SamplerLocalPermutation (gat/Engine.pyx:1117-1229) through the C ABI against tests/local_permutation_model.py --
the reference's walk on CPython's random.Random, pinned to the reference's own output by
tests/test_local_permutation_model.py.  Bit-exact: the sampled (sample, unit) lists, the words drawn and the count
matrices."""
import importlib.util
import json
import os
import random

import numpy as np
import pytest

import gat_amd
import local_permutation_edges as LE
import local_permutation_model as M
from gat_amd import _lib, problem, synthetic

pytestmark = pytest.mark.gpu
INT_COUNTERS = ["nucleotide-overlap", "segment-overlap", "segment-midoverlap", "annotation-overlap"]


@pytest.fixture(scope="module", params=["batched", "simple"])
def ctx(request):
    """both variants of k_permute_local: small pieces resolved in batches (the default), and one piece per wave step
    (context option GAT_LPERM_SIMPLE)."""
    c = _lib.Context(0)
    if request.param == "simple":
        c.options["GAT_LPERM_SIMPLE"] = "1"
    yield c
    c.close()


def _check(ctx, flat, seed, s0, s1):
    got, st = LE.device_units(ctx, flat, seed, s0, s1)
    want, wst = LE.model_units(flat, seed, s0, s1)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:6], w[:6])
    assert st["n_draws"] == wst["n_draws"]
    return want


def test_kats_exact():
    """the reference's own single-unit known answers (tests/golden/local_permutation/kat.json) through
    SamplerLocalPermutation.sample: the list, or an error where the reference raised."""
    sampler = gat_amd.SamplerLocalPermutation()
    cases = M.load_kats()
    for i, c in enumerate(cases):
        segs = gat_amd.SegmentList(iter=c["segments"], normalize=True)
        ws = gat_amd.SegmentList(iter=c["workspace"], normalize=True)
        if c["error"]:
            with pytest.raises(AssertionError):
                sampler.sample(segs, ws, seed=c["seed"])
            continue
        a = sampler.sample(segs, ws, seed=c["seed"]).asArray()
        assert [(int(s), int(e)) for s, e in zip(a["start"], a["end"])] == c["sample"], i


@pytest.mark.parametrize("seed", LE.SEEDS)
def test_units_vs_model(ctx, seed):
    """random units (a third with fragmented workspaces of hundreds of pieces) x samples: every (sample, unit) list and
    the number of 32-bit words drawn."""
    flat = LE.units_flat(LE.random_units(random.Random(seed), LE.N_RANDOM_UNITS))
    want = _check(ctx, flat, seed, 0, LE.N_SAMPLES)
    assert sum(map(len, want)) > 0


def test_split_sample_ranges(ctx):
    """samples [5, 13) in one call equal the same samples of the model (the stream is per (sample, unit))."""
    flat = LE.units_flat(LE.random_units(random.Random(9), 30))
    _check(ctx, flat, 42, 5, 13)


@pytest.mark.parametrize("name", [n for n, _ in LE.fixed_units()])
def test_fixed_units(ctx, name):
    """long_list: a final list beyond the LDS bound (sorted and merged in the slab) beside a short unit; long_piece: more
    than 2 048 working segments in ONE piece (lengths and points in the slab); small_pieces: several thousand active
    pieces of one or two segments; edges: the hand-made shapes."""
    units = dict(LE.fixed_units())[name]
    flat = LE.units_flat(units)
    want = _check(ctx, flat, 3, 0, 2)
    tables = [M.unit_tables(s, w) for s, w in units]
    if name == "long_list":
        assert max(len(x) for x in want) > LE.LDS_LIST and max(t[1] for tt in tables for t in tt) <= LE.LDS_LIST
    if name == "long_piece":
        assert max(t[1] for tt in tables for t in tt) > LE.LDS_LIST
    if name == "small_pieces":
        assert len(tables[0]) >= 3000 and max(t[1] for t in tables[0]) <= 3


def _genome_flat(isochores):
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"] if isochores else None)
    flat["sampler"] = LE.LOCAL
    return flat


@pytest.mark.parametrize("isochores", [False, True])
def test_counts_vs_model(ctx, isochores):
    """a whole problem: (sample, unit) lists and the count matrices, with and without isochores; a sample range split
    over calls gives the same matrix."""
    flat = _genome_flat(isochores)
    S = 12
    want_lists = LE.model_units(flat, 77, 0, S)[0]
    want = LE.model_counts(flat, want_lists, INT_COUNTERS, S)
    assert LE.device_units(ctx, flat, 77, 0, S)[0] == want_lists
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(INT_COUNTERS, 77, 0, S)
        parts = [P.sample_and_count(INT_COUNTERS, 77, a, b) for a, b in ((0, 5), (5, 12))]
    finally:
        P.close()
    for k, c in enumerate(INT_COUNTERS):
        assert np.array_equal(got[k], want[k]), c
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), want[k]), c


def test_reference_stream_refused_by_the_library(ctx):
    """GAT_ERR_ARG (ValueError), with the sampler named."""
    P = _lib.Problem(ctx, _genome_flat(False))
    try:
        state = np.zeros(_lib.MT_STATE_WORDS, dtype=np.uint32)
        state[-1] = 624
        with pytest.raises(ValueError, match="SamplerLocalPermutation"):
            P.sample_and_count_serial(INT_COUNTERS, state, 4)
    finally:
        P.close()


def test_overflow_in_a_batch(ctx):
    """units near 2^31 whose walk leaves 2^31 - 1 for some (sample, unit) only -- two consecutive pieces of one working
    segment, pieces of one and of two (the batched draw path), a piece of three (the piece-by-piece path) -- beside
    ordinary units: a sample range in which the model raises OverflowError is refused with AssertionError, one in which
    it does not is sampled exactly."""
    big = 2 ** 31 - 1
    r = random.Random(5)
    risky = [([(50, 60)], [(100, 200), (big - 2000, big - 1)]),
             ([(50, 60), (big - 1000, big - 10)], [(100, 200), (big - 2000, big - 1)]),
             ([(100, 200), (300, 400), (big - 800, big - 10)], [(0, big - 1)])]
    assert [[t[1] for t in M.unit_tables(*u)] for u in risky] == [[1, 1], [1, 2], [3]]
    for unit in risky:
        flat = LE.units_flat(LE.random_units(r, 3) + [unit] + LE.random_units(r, 2))
        n, u = int(flat["n_units"]), 3
        raises = []
        for s in range(24):
            try:
                M.sample(random.Random((11 + s * n + u) & 0xFFFFFFFF), *unit)
                raises.append(False)
            except OverflowError:
                raises.append(True)
        assert any(raises) and not all(raises)
        bad = raises.index(True)
        with pytest.raises(AssertionError, match="2\\^31"):
            LE.device_units(ctx, flat, 11, max(0, bad - 2), bad + 3)
        runs = [(a, b) for a in range(24) for b in range(a + 1, 25) if not any(raises[a:b])]
        a, b = max(runs, key=lambda ab: ab[1] - ab[0])
        _check(ctx, flat, 11, a, b)


def test_negative_free_refused_at_problem_creation(ctx):
    """working segments longer than [0, piece end): the reference's randint raises; the library refuses the problem."""
    with pytest.raises(AssertionError):
        _lib.Problem(ctx, LE.units_flat([([(30, 45)], [(0, 100)]), ([(0, 40), (40, 101)], [(0, 100)])]))


def test_cli_tables_byte_equal(tmp_path):
    """scripts/gat-run.py --sampler=local-permutation prints the reference's table (per-unit stream patch) byte for byte:
    plain, isochores, several segment tracks, a conditional workspace."""
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("gat_run_cli", os.path.join(here, "..", "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cli_in, gold = os.path.join(here, "golden", "cli"), os.path.join(here, "golden", "local_permutation", "cli")
    cases = json.load(open(os.path.join(gold, "cases.json")))
    assert len(cases) == 4
    for name, extra in cases.items():
        extra = [x.replace("--isochores=", "--isochores=%s%s" % (cli_in, os.sep)) for x in extra]
        out = str(tmp_path / ("%s.tsv" % name))
        argv = ["gat-run.py", "--segments=%s" % os.path.join(cli_in, "segments.bed"),
                "--annotations=%s" % os.path.join(cli_in, "annotations.bed"),
                "--workspace=%s" % os.path.join(cli_in, "workspace.bed"), "--stdout=%s" % out,
                "--log=%s" % str(tmp_path / "log")] + extra
        assert mod.main(argv) == 0
        got = [l for l in open(out) if not l.startswith("#")]
        want = [l for l in open(os.path.join(gold, "expected_%s.tsv" % name))]
        assert got == want, name
