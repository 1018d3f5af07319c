"""GPU: SamplerGlobalPermutation (gat/Engine.pyx:1234-1386) through the C ABI against tests/permutation_model.py -- the
reference's walk in closed form on CPython's random.Random, pinned to the reference's own output by
tests/test_permutation_model.py.  Bit-exact: the sampled (sample, unit) lists and the count matrices."""
import importlib.util
import json
import os
import random

import numpy as np
import pytest

import gat_amd
import permutation_model as M
import sampler_edges as E
from gat_amd import _lib, problem, synthetic

pytestmark = pytest.mark.gpu
INT_COUNTERS = ["nucleotide-overlap", "segment-overlap", "segment-midoverlap", "annotation-overlap"]
KIND = E.PERM


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


_rand_norm, _as_lists, _model_counts = E.rand_norm, E.as_lists, E.model_counts


def _units_flat(units):
    return E.units_flat(units, KIND)


def _model_units(flat, seed, s0, s1):
    """the model's (sample, unit) lists in gat_sample_units' order: unit u of sample s draws from
    random.seed((seed + s * n_units + u) mod 2^32)."""
    return E.model_units(flat, seed, s0, s1)[0]


def _device_units(ctx, flat, seed, s0, s1):
    return E.device_units(ctx, flat, seed, s0, s1)


def _random_units(r, n, fragmented=0.3):
    units = []
    for _ in range(n):
        span = r.choice([200, 1000, 5000, 40000])
        segs = _rand_norm(r, r.randint(1, 40), span, r.choice([1, 5, 50, 400]))
        if r.random() < fragmented:      # fragmented workspace: hundreds of short pieces
            n_ws = r.randint(100, 400)
            ws = _rand_norm(r, n_ws, max(span, 10 * n_ws) + 100, r.choice([2, 5, 20]))
        else:
            ws = _rand_norm(r, r.randint(1, 20), span + 100, r.choice([1, 3, 30, 2000]))
        units.append((segs, ws))
    return units


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 32 - 3])
def test_units_vs_model(ctx, seed):
    """80 random units (a third with fragmented workspaces) x 6 samples: every (sample, unit) list."""
    flat = _units_flat(_random_units(random.Random(seed), 80))
    got, st = _device_units(ctx, flat, seed, 0, 6)
    want = _model_units(flat, seed, 0, 6)
    assert sum(map(len, want)) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:6], w[:6])
    assert st["n_draws"] > 0


def test_split_sample_ranges(ctx):
    """samples [5, 13) in one call equal the same samples of the model (the stream is per (sample, unit))."""
    flat = _units_flat(_random_units(random.Random(9), 30))
    got, _ = _device_units(ctx, flat, 42, 5, 13)
    assert got == _model_units(flat, 42, 5, 13)


def test_fragmented_units(ctx):
    """every unit fragmented: hundreds of workspace pieces, segments bridging and overhanging them."""
    flat = _units_flat(_random_units(random.Random(11), 24, fragmented=1.0))
    got, _ = _device_units(ctx, flat, 5, 0, 4)
    assert got == _model_units(flat, 5, 0, 4)


def test_unit_longer_than_lds(ctx):
    """units of 2 500 and 4 000 working segments (beyond the 2 048 the LDS buffers hold: lengths and points in the slab)
    beside a short one."""
    r = random.Random(3)
    long1 = (_rand_norm(r, 2500, 2_000_000, 300), _rand_norm(r, 30, 2_100_000, 200_000))
    long2 = (_rand_norm(r, 4000, 3_000_000, 200), [(0, 3_100_000)])
    short = (_rand_norm(r, 20, 5000, 50), [(0, 5100)])
    flat = _units_flat([long1, short, long2])
    got, _ = _device_units(ctx, flat, 77, 0, 3)
    want = _model_units(flat, 77, 0, 3)
    assert max(len(x) for x in want) > 2048
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i


def _genome_flat(isochores):
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"] if isochores else None)
    flat["sampler"] = KIND
    return flat


@pytest.mark.parametrize("isochores", [False, True])
def test_counts_vs_model(ctx, isochores):
    """a whole problem: (sample, unit) lists and the count matrices, with and without isochores; a sample range split
    over calls gives the same matrix."""
    flat = _genome_flat(isochores)
    S = 12
    want_lists = _model_units(flat, 77, 0, S)
    want = _model_counts(flat, want_lists, INT_COUNTERS, S)
    assert _device_units(ctx, flat, 77, 0, S)[0] == want_lists
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
    P = _lib.Problem(ctx, _genome_flat(False))
    try:
        state = np.zeros(_lib.MT_STATE_WORDS, dtype=np.uint32)
        state[-1] = 624
        with pytest.raises(Exception):
            P.sample_and_count_serial(INT_COUNTERS, state, 4)
    finally:
        P.close()


def test_kats_exact():
    """the reference's own single-unit known answers (tests/golden/permutation/kat.json) through
    SamplerGlobalPermutation.sample."""
    sampler = gat_amd.SamplerGlobalPermutation()
    cases = M.load_kats()
    for i, c in enumerate(cases):
        got = sampler.sample(gat_amd.SegmentList(iter=c["segments"], normalize=True),
                             gat_amd.SegmentList(iter=c["workspace"], normalize=True), seed=c["seed"])
        a = got.asArray()
        assert [(int(s), int(e)) for s, e in zip(a["start"], a["end"])] == c["sample"], i


def test_cli_tables_byte_equal(tmp_path):
    """scripts/gat-run.py --sampler=global-permutation prints the reference's table (per-unit stream patch) byte for byte:
    plain, isochores, several segment tracks, a conditional workspace."""
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("gat_run_cli", os.path.join(here, "..", "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cli_in, gold = os.path.join(here, "golden", "cli"), os.path.join(here, "golden", "permutation", "cli")
    cases = json.load(open(os.path.join(gold, "cases.json")))
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
