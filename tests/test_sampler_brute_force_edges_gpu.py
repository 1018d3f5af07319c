"""GPU: k_brute_force through the edge cases of tests/brute_force_edges.py, bit-exact against tests/brute_force_model.py:
every (sample, unit) list, the words each stream consumed (n_draws), restarts, placements and rejections; all six
counters; calls cut into many batches, the enqueue / wait seam, the slab-overflow retry, the non-convergence status
across batches and a launch of more units than a grid dimension.  tests/test_brute_force_edges.py shows on the model
which branches these calls reach."""
import numpy as np
import pytest

import brute_force_edges as B
import brute_force_model as M
from gat_amd import _lib, problem, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _check_units(ctx, flat, seed, s0, s1):
    want, mst = B.model_units(flat, seed, s0, s1)
    assert mst["unconverged"] == 0
    got, st = B.device_units(ctx, flat, seed, s0, s1)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(g), len(w), [(a, b) for a, b in zip(g, w) if a != b][:4])
    B.check_stats(st, mst)
    return st


def brute_case(ctx, seed):
    """brute-force case `seed` (tools/fuzz_sweep.py brute): 4 samples from a seed-dependent base."""
    _check_units(ctx, *B.fuzz_call(seed))


@pytest.mark.parametrize("seed", list(range(B.N_SEEDS)))
def test_brute_fuzz(ctx, seed):
    brute_case(ctx, seed)


@pytest.mark.parametrize("name", [c["name"] for c in B.fixed_units()])
def test_brute_fixed(ctx, monkeypatch, name):
    """one hand-built case per k_brute_force branch (brute_force_edges.fixed_units) on 3 samples."""
    case = [c for c in B.fixed_units() if c["name"] == name][0]
    flat = B.units_flat(case["units"], **case["params"])
    for k, v in case["knobs"].items():
        monkeypatch.setitem(ctx.options, k, v)
    if case["error"]:
        # the reference's outcome as the known answers record it: ValueError for every recorded seed (sample 0 of a
        # one-unit call with the known answer's seed draws from that very stream)
        kats = [k for k in M.load_kats() if k["segments"] == case["units"][0][0] and k["workspace"] == case["units"][0][1]]
        assert len(kats) == 6
        P = _lib.Problem(ctx, flat)
        try:
            for k in kats:
                assert k["error"] == "ValueError"
                with pytest.raises(ValueError, match="did not converge"):
                    P.sample(k["seed"], 0, 1, unit_level=True)
                assert P.last_stats["n_unconverged"] == 1
                assert "sample 0, unit 0" in _lib.lib().gat_last_error(ctx._h).decode()
        finally:
            P.close()
        return
    st = _check_units(ctx, flat, case["seed"], 0, B.FIXED_SAMPLES)
    assert (st["n_retried"] > 0) == case["retried"], st["n_retried"]


def _genome_flat():
    """synthetic.small_genome without isochores, every fourth segment, cut to 1 or 2 bases (so that the units converge):
    the segment-shortening of tests/test_sampler_brute_force.py"""
    _, cfg = synthetic.small_genome()
    segs = cfg["segments"]
    for c in segs:
        a = segs[c][::4].copy()
        a["end"] = a["start"] + 1 + (a["end"] - a["start"] - 1) % 2
        segs[c] = a
    flat = problem.flatten_arrays(segs, cfg["annotations"], cfg["workspace"], None, bucket_size=1)
    flat["sampler"] = B.BRUTE
    return flat


@pytest.fixture(scope="module")
def genome():
    """the genome problem and the model's lists, statistics and counts of samples [3, 43) under seed 8 (computed once)."""
    flat = _genome_flat()
    assert int(flat["merge_contigs"]) == 0
    lists, mst = B.model_units(flat, 8, 3, 43)
    assert mst["unconverged"] == 0
    return dict(flat=flat, lists=lists, mst=mst, counts=B.model_counts(flat, lists, B.E.ALL_COUNTERS, 40))


def test_all_counters_vs_model(ctx, genome):
    """the six counters (nucleotide-density exact in float64) over a whole problem without isochores."""
    P = _lib.Problem(ctx, genome["flat"])
    try:
        got = P.sample_and_count(B.E.ALL_COUNTERS, 8, 3, 13)
    finally:
        P.close()
    for k, c in enumerate(B.E.ALL_COUNTERS):
        assert got[k].dtype == genome["counts"][k].dtype and np.array_equal(got[k], genome["counts"][k][:, :10]), c


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


def _slab_bytes(ctx, flat, samples):
    """a GAT_SLAB_BYTES under which a batch holds at most `samples` samples (the budget over the slab's 8 bytes per entry;
    what else a sample takes only makes the batch smaller)."""
    P = _lib.Problem(ctx, flat)
    try:
        return str(int((samples + 0.5) * 8 * P.info()["slab_segments_per_sample"]))
    finally:
        P.close()


def test_many_batches_and_the_seam(ctx, monkeypatch, genome):
    """batches of at most 4 of the call's 40 samples (sample_begin differs per batch): the enqueue / wait seam, the
    blocking call and the unit-level call agree with the model, and the four statistics summed over the batches are the
    model's."""
    flat, want = genome["flat"], genome["counts"]
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", _slab_bytes(ctx, flat, 4))
    P = _lib.Problem(ctx, flat)
    try:
        got, st = _enqueue_wait(ctx, P, B.E.ALL_COUNTERS, 8, 3, 43)
        assert st["n_batches"] > 8, st
        blocking = P.sample_and_count(B.E.ALL_COUNTERS, 8, 3, 43)
        bst = P.last_stats
        assert bst["n_batches"] > 8
        seg, off = P.sample(8, 3, 43, unit_level=True)
        ust = P.last_stats
    finally:
        P.close()
    for k, c in enumerate(B.E.ALL_COUNTERS):
        assert np.array_equal(got[k], want[k]), c
        assert np.array_equal(blocking[k], want[k]), c
    assert B.as_lists(seg, off) == genome["lists"]
    for s in (st, bst, ust):
        B.check_stats(s, genome["mst"])


def test_retry_in_many_batches(ctx, monkeypatch):
    """GAT_TEST_SMALL_CAPS with a small scratch budget: batches overflow and are laid out again.  The lists equal the
    model's, and the statistics over the call's batches are counted once."""
    units = B.edge_units(9)[0] + [B.ones(130), B.ones_and_outside(129, 5)]
    flat = B.units_flat(units, **B.edge_units(9)[1])
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", _slab_bytes(ctx, flat, 4))
    _check_units(ctx, flat, 31, 0, 12)
    # (the unit-level call may be repeated with a larger host buffer, its last statistics then show no retry: the
    #  retries and batches are read from a counting call)
    _, mst = B.model_units(flat, 31, 0, 12)
    P = _lib.Problem(ctx, flat)
    try:
        P.sample_and_count(["nucleotide-overlap"], 31, 0, 12)
        st = P.last_stats
    finally:
        P.close()
    assert st["n_retried"] > 0 and st["n_batches"] > 2, st
    B.check_stats(st, mst)


def _two_piece_unit(k, w):
    """30 segments of 1-2 bases in two pieces of 310 and w bases: with 3 tries and 2 passes one (sample, unit) in some
    dozens does not converge"""
    return [(100 + 10 * i, 100 + 10 * i + 1 + (i + k) % 2) for i in range(30)], [(90, 400), (400 + w, 400 + 2 * w)]


def test_non_convergence_across_batches(ctx, monkeypatch):
    """ntries_inner=3, ntries_outer=2 on four units, 12 samples in batches of at most 2.  The model has (sample 2, unit 3)
    and (sample 11, unit 0) unconverged: two batches, two units.  The call fails at the first batch that holds one --
    batches are checked in order, the later ones are never looked at -- and names the first pair of it in sample-major
    order, which is the first of the call; n_unconverged is that batch's count.  (A status path, not a fault.)"""
    units = [_two_piece_unit(0, 150), ([(5, 6), (9, 10)], [(0, 50)]), _two_piece_unit(1, 250), _two_piece_unit(2, 100)]
    flat = B.units_flat(units, ntries_inner=3, ntries_outer=2)
    n, seed = 4, 83
    lists, _ = B.model_units(flat, seed, 0, 12)
    bad = [(i // n, i % n) for i, l in enumerate(lists) if l is None]
    assert bad == [(2, 3), (11, 0)]
    first = "sample %d, unit %d" % bad[0]
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", _slab_bytes(ctx, flat, 2))
    P = _lib.Problem(ctx, flat)
    try:
        # a converging range in many batches first: the batch size is what this test needs
        P.sample_and_count(["nucleotide-overlap"], seed, 3, 11)
        assert P.last_stats["n_batches"] >= 4, P.last_stats
        for call in (lambda: P.sample_and_count(["nucleotide-overlap"], seed, 0, 12),
                     lambda: P.sample(seed, 0, 12, unit_level=True)):
            with pytest.raises(ValueError, match="did not converge"):
                call()
            msg = _lib.lib().gat_last_error(ctx._h).decode()
            assert first in msg, msg
            # (the failed batch begins at sample 2 at the latest and ends before sample 11: one pair)
            assert P.last_stats["n_unconverged"] == 1
        # the later pair alone: named when the range begins behind the first
        with pytest.raises(ValueError, match="did not converge"):
            P.sample(seed, 3, 12, unit_level=True)
        assert "sample 11, unit 0" in _lib.lib().gat_last_error(ctx._h).decode()
        # the problem goes on working: a converging range still matches the model
        seg, off = P.sample(seed, 3, 11, unit_level=True)
        want, mst = B.model_units(flat, seed, 3, 11)
        assert B.as_lists(seg, off) == want
        B.check_stats(P.last_stats, mst)
    finally:
        P.close()


def test_more_units_than_a_grid_dimension(ctx):
    """66 000 units of one 1-base segment in a piece of 2 bases, 1 sample: the launch's grid is (1, 32 768, 3) and the unit
    is blockIdx.y + blockIdx.z * gridDim.y.  The model takes 0.3 ms per unit, so 2 070 of the 66 000 lists are compared --
    every 33rd unit, the first, the last, 32 750 .. 32 790 and 65 520 .. 65 550 -- and the lengths of all; the call's n_draws is compared
    with 2 words per unit: randint(0, 2) and randint(x, x + 2) take one word each whatever the stream (ranges of 2^k: no
    rejection), as the 2 000 modelled units show."""
    N, seed = 66000, 7
    units = [([(5 * u + u % 2, 5 * u + u % 2 + 1)], [(5 * u, 5 * u + 2)]) for u in range(N)]
    flat = B.units_flat(units)
    picked = sorted(set(range(0, N, 33)) | {0, N - 1} | set(range(32750, 32791)) | set(range(65520, 65551)))
    assert len(picked) >= 2000
    got, st = B.device_units(ctx, flat, seed, 0, 1)
    assert len(got) == N and all(len(g) == 1 for g in got)
    for u in picked:
        rng = O.RandomState((seed + u) & 0xFFFFFFFF)
        want = M.sample(rng, *units[u])
        assert got[u] == want, (u, got[u], want)
        assert rng.ndraws == 2
    assert st["n_draws"] == 2 * N and st["n_placed"] == N and st["n_restarts"] == 0 and st["n_unconverged"] == 0
