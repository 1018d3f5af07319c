"""GPU: k_shift and k_permute through the edge cases of tests/sampler_edges.py, bit-exact against the models: every
(sample, unit) list, the words each stream consumed (n_draws) and the shift's empty windows; all six counters; calls
cut into many batches, the enqueue / wait seam and the slab-overflow retry."""
import numpy as np
import pytest

import sampler_edges as E
from gat_amd import _lib, problem, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _check_units(ctx, flat, seed, s0, s1):
    got, st = E.device_units(ctx, flat, seed, s0, s1)
    want, mst = E.model_units(flat, seed, s0, s1)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(g), len(w), [(a, b) for a, b in zip(g, w) if a != b][:4])
    assert st["n_draws"] == mst["n_draws"], (st["n_draws"], mst["n_draws"])
    if int(flat["sampler"]) == E.SHIFT:
        assert st["n_empty_windows"] == mst["n_empty_windows"]
    return st


def shift_case(ctx, seed):
    """shift case `seed` (tools/fuzz_sweep.py shift): 4 samples from a seed-dependent base."""
    units, radius, extension = E.shift_edge_units(seed)
    _check_units(ctx, E.units_flat(units, E.SHIFT, radius, extension), 1000 + 7919 * seed, 3, 7)


def perm_case(ctx, seed):
    """permutation case `seed` (tools/fuzz_sweep.py perm): 4 samples from a seed-dependent base."""
    _check_units(ctx, E.units_flat(E.perm_edge_units(seed), E.PERM), 2000 + 104729 * seed, 3, 7)


@pytest.mark.parametrize("seed", list(range(48)))
def test_shift_fuzz(ctx, seed):
    shift_case(ctx, seed)


@pytest.mark.parametrize("seed", list(range(48)))
def test_perm_fuzz(ctx, seed):
    perm_case(ctx, seed)


@pytest.mark.parametrize("name", [x[0] for x in E.shift_fixed_units()])
def test_shift_fixed(ctx, name):
    """one hand-built case per k_shift branch (sampler_edges.shift_fixed_units)."""
    _, units, radius, extension = [x for x in E.shift_fixed_units() if x[0] == name][0]
    _check_units(ctx, E.units_flat(units, E.SHIFT, radius, extension), 99, 0, 3)


@pytest.mark.parametrize("name", [x[0] for x in E.perm_fixed_units()])
def test_perm_fixed(ctx, name):
    """one hand-built case per k_permute branch (sampler_edges.perm_fixed_units): 2 048 / 2 049 alone and mixed,
    n = 1 / 63 / 64 / 65 / 128 / 129, free = 0 and large, W in 1-2 base pieces."""
    units = [x for x in E.perm_fixed_units() if x[0] == name][0][1]
    _check_units(ctx, E.units_flat(units, E.PERM), 4242, 0, 3)


def _genome_flat(kind, isochores):
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], cfg["annotations"], cfg["workspace"], cfg["isochores"] if isochores else None)
    flat["sampler"] = kind
    if kind == E.SHIFT:
        flat["shift_radius"], flat["shift_extension"] = 2.0, 0
    return flat


def _enqueue_wait(ctx, P, counters, seed, lo, hi):
    dev = ctx.alloc(max(1, len(counters) * P.n_tracks * (hi - lo)) * 8)
    try:
        P.enqueue(counters, seed, lo, hi, dev)
        st = P.wait()
        host = np.empty((len(counters), P.n_tracks, hi - lo), dtype=np.int64)
        if host.size:
            ctx.d2h(host, dev)
    finally:
        ctx.free(dev)
    return [host[k].view(np.float64) if c == "nucleotide-density" else host[k] for k, c in enumerate(counters)], st


@pytest.mark.parametrize("kind", [E.SHIFT, E.PERM])
@pytest.mark.parametrize("isochores", [False, True])
def test_all_counters_vs_model(ctx, kind, isochores):
    """the six counters (nucleotide-density exact in float64) over whole problems, against the model's lists."""
    flat = _genome_flat(kind, isochores)
    S = 10
    want_lists, _ = E.model_units(flat, 55, 0, S)
    want = E.model_counts(flat, want_lists, E.ALL_COUNTERS, S)
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(E.ALL_COUNTERS, 55, 0, S)
    finally:
        P.close()
    for k, c in enumerate(E.ALL_COUNTERS):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), c


@pytest.mark.parametrize("kind", [E.SHIFT, E.PERM])
def test_many_batches_and_the_seam(ctx, monkeypatch, kind):
    """a scratch budget of a few samples: the call is many batches (sample_begin differs per batch); the blocking call,
    the enqueue / wait seam and the model agree, and so do the lists and draws of a unit-level call cut the same way."""
    flat = _genome_flat(kind, True)
    S = 40
    want_lists, mst = E.model_units(flat, 8, 3, 3 + S)
    want = E.model_counts(flat, want_lists, E.ALL_COUNTERS, S)
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "40000")
    P = _lib.Problem(ctx, flat)
    try:
        got, st = _enqueue_wait(ctx, P, E.ALL_COUNTERS, 8, 3, 3 + S)
        assert st["n_batches"] > 8, st
        blocking = P.sample_and_count(E.ALL_COUNTERS, 8, 3, 3 + S)
        assert P.last_stats["n_batches"] > 8
        seg, off = P.sample(8, 3, 3 + S, unit_level=True)
        ust = P.last_stats
        assert ust["n_batches"] > 8, ust
    finally:
        P.close()
    for k, c in enumerate(E.ALL_COUNTERS):
        assert np.array_equal(got[k], want[k]), c
        assert np.array_equal(blocking[k], want[k]), c
    assert E.as_lists(seg, off) == want_lists
    assert ust["n_draws"] == mst["n_draws"]
    if kind == E.SHIFT:
        assert ust["n_empty_windows"] == mst["n_empty_windows"]


def test_shift_retry_in_many_batches(ctx, monkeypatch):
    """GAT_TEST_SMALL_CAPS with a small scratch budget: batches overflow and are laid out again.  The lists equal the
    model's, and so do the call's draws and empty windows over its batches (a redone batch is not counted twice)."""
    units, radius, extension = E.shift_edge_units(14)
    units += [x[1][0] for x in E.shift_fixed_units() if x[0] in ("fill_all_lanes", "near_zero")]
    flat = E.units_flat(units, E.SHIFT, radius, extension)
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "300000")
    _check_units(ctx, flat, 31, 0, 12)
    # (the unit-level call may be repeated with a larger host buffer, its last statistics then show no retry: the
    #  retries and batches are read from a counting call)
    _, mst = E.model_units(flat, 31, 0, 12)
    P = _lib.Problem(ctx, flat)
    try:
        P.sample_and_count(["nucleotide-overlap"], 31, 0, 12)
        st = P.last_stats
    finally:
        P.close()
    assert st["n_retried"] > 0 and st["n_batches"] > 2, st
    assert st["n_draws"] == mst["n_draws"] and st["n_empty_windows"] == mst["n_empty_windows"] > 0
