"""GPU: SamplerShift (gat/Engine.pyx:998-1111) through the C ABI against tests/shift_model.py -- the reference's
walk restated on the oracle's RandomState, pinned to the reference's own output by tests/test_shift_model.py.
Bit-exact: the sampled (sample, unit) lists and the count matrices."""
import random

import numpy as np
import pytest

import sampler_edges as E
import shift_model as M
from gat_amd import _lib, problem, synthetic

pytestmark = pytest.mark.gpu
INT_COUNTERS = ["nucleotide-overlap", "segment-overlap", "segment-midoverlap", "annotation-overlap"]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


_rand_norm, _as_lists, _model_counts = E.rand_norm, E.as_lists, E.model_counts


def _units_flat(units, radius, extension):
    return E.units_flat(units, E.SHIFT, radius, extension)


def _model_units(flat, seed, s0, s1):
    """the model's (sample, unit) lists and its empty-window count, in gat_sample_units' order."""
    lists, st = E.model_units(flat, seed, s0, s1)
    return lists, st["n_empty_windows"]


def _device_units(ctx, flat, seed, S):
    """the library's (sample, unit) lists of samples [0, S) and the call's statistics."""
    return E.device_units(ctx, flat, seed, 0, S)


def _random_units(r, n):
    units = []
    for _ in range(n):
        span = r.choice([200, 1000, 5000, 40000])
        segs = _rand_norm(r, r.randint(1, 14), span, r.choice([1, 5, 50, 400]))
        if r.random() < 0.3:      # fragmented workspace: hundreds of short pieces
            n_ws = r.randint(100, 400)
            ws = _rand_norm(r, n_ws, max(span, 10 * n_ws) + 100, r.choice([2, 5, 20]))
        else:
            ws = _rand_norm(r, r.randint(1, 20), span + 100, r.choice([1, 3, 30, 2000]))
        units.append((segs, ws))
    return units


@pytest.mark.parametrize("radius,extension", [(2.0, 0), (0.5, 0), (3.7, 0), (1.0, 7), (2.0, 200), (2.0, 500)])
def test_units_vs_model(ctx, radius, extension):
    """60 random units (segments near 0, small / fragmented / empty windows) x 5 samples: lists and draws."""
    r = random.Random(int(radius * 10) * 1000 + extension)
    flat = _units_flat(_random_units(r, 60), radius, extension)
    got, st = _device_units(ctx, flat, 1234, 5)
    want, empty = _model_units(flat, 1234, 0, 5)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert st["n_empty_windows"] == empty


def test_empty_windows_counted(ctx):
    """radius 0: every window is empty -- nothing placed, one draw (the direction) per segment, the run succeeds."""
    units = [([(10, 50), (60, 61), (100, 300)], [(0, 1000)]), ([(5, 6)], [(0, 10), (20, 30)])]
    got, st = _device_units(ctx, _units_flat(units, 0.0, 0), 7, 4)
    assert not any(got)
    assert st["n_empty_windows"] == 4 * 4 and st["n_draws"] == 4 * 4


def _genome_flat(isochores):
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"] if isochores else None)
    flat["sampler"], flat["shift_radius"], flat["shift_extension"] = 2, 2.0, 0
    return flat


@pytest.mark.parametrize("isochores", [False, True])
def test_counts_vs_model(ctx, isochores):
    """a whole problem: (sample, unit) lists and the count matrices, with and without isochores."""
    flat = _genome_flat(isochores)
    S = 12
    want_lists, _ = _model_units(flat, 77, 0, S)
    want = _model_counts(flat, want_lists, INT_COUNTERS, S)
    assert _device_units(ctx, flat, 77, S)[0] == want_lists
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(INT_COUNTERS, 77, 0, S)
        # a sample range split over calls gives the same matrix
        parts = [P.sample_and_count(INT_COUNTERS, 77, a, b) for a, b in ((0, 5), (5, 12))]
    finally:
        P.close()
    for k, c in enumerate(INT_COUNTERS):
        assert np.array_equal(got[k], want[k]), c
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), want[k]), c


def test_slab_overflow_retry(ctx):
    """GAT_TEST_SMALL_CAPS: regions of half a unit's segments -- the batch overflows, the slab is laid out again."""
    r = random.Random(5)
    flat = _units_flat(_random_units(r, 24), 2.0, 500)
    ctx.options["GAT_TEST_SMALL_CAPS"] = "1"
    try:
        got, st = _device_units(ctx, flat, 3, 6)
    finally:
        ctx.options.pop("GAT_TEST_SMALL_CAPS", None)
    want, mst = E.model_units(flat, 3, 0, 6)
    assert got == want
    assert st["n_retried"] > 0
    # the redone batches' draws and empty windows are counted once
    assert st["n_draws"] == mst["n_draws"] and st["n_empty_windows"] == mst["n_empty_windows"]


def test_rejections(ctx):
    """no reference-stream mode for SamplerShift; a negative radius or extension is refused at problem creation."""
    flat = _genome_flat(False)
    P = _lib.Problem(ctx, flat)
    try:
        state = np.zeros(_lib.MT_STATE_WORDS, dtype=np.uint32)
        state[-1] = 624
        with pytest.raises(Exception):
            P.sample_and_count_serial(INT_COUNTERS, state, 4)
    finally:
        P.close()
    for radius, extension in ((-1.0, 0), (2.0, -4)):
        flat["shift_radius"], flat["shift_extension"] = radius, extension
        with pytest.raises(Exception):
            _lib.Problem(ctx, flat)


def test_kats_exact(ctx):
    """the reference's own single-unit known answers (tests/golden/shift/kat.json), one problem per parameter pair."""
    by_param = {}
    for c in M.load_kats():
        by_param.setdefault((c["radius"], c["extension"]), []).append(c)
    for (radius, extension), group in by_param.items():
        P = _lib.Problem(ctx, _units_flat([(c["segments"], c["workspace"]) for c in group], radius, extension))
        try:
            for i, c in enumerate(group):
                # unit i of sample 0 draws from seed + i: the base seed is chosen so that it gets c["seed"]
                seg, off = P.sample((c["seed"] - i) & 0xFFFFFFFF, 0, 1, unit_level=True)
                assert _as_lists(seg, off)[i] == c["sample"], (radius, extension, i)
        finally:
            P.close()


def test_cli_tables_byte_equal(tmp_path):
    """scripts/gat-run.py --sampler=shift prints the reference's table (per-unit stream patch) byte for byte."""
    import importlib.util
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("gat_run_cli", os.path.join(here, "..", "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cli_in, gold = os.path.join(here, "golden", "cli"), os.path.join(here, "golden", "shift", "cli")
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
