"""CPU: tests/local_permutation_model.py (SamplerLocalPermutation on random.Random) == the reference's own
SamplerLocalPermutation on the known-answer cases of tests/golden/local_permutation/kat.json -- the sampled list and what
the sample consumed of the stream, or the exception the reference raised -- and the known answers and the GPU tests'
generated units reach every event the feature's conditions list."""
import random

import pytest

import local_permutation_edges as LE
import local_permutation_model as M

# the events every set of cases has to reach at least once (local_permutation_model.sample's stats)
EVENTS = ["lone_not_overlapping", "shared_segment", "united", "adjacent_apart", "end_on_work_end", "start_on_work_end",
          "wrapped_segment", "wrapped_start", "free_is_0", "n_is_1", "n_above_64", "bound_pow2", "bound_above_pow2",
          "idle_then_active", "adjacent_ws", "output_without_filter", "empty_result", "near_2_31"]


def test_model_matches_reference_kats():
    cases = M.load_kats()
    assert len(cases) >= 500
    raised = 0
    for i, c in enumerate(cases):
        rng = random.Random(c["seed"])
        if c["error"]:
            with pytest.raises((ValueError, OverflowError)) as e:
                M.sample(rng, c["segments"], c["workspace"])
            assert type(e.value).__name__ == c["error"], i
            raised += 1
            continue
        got = M.sample(rng, c["segments"], c["workspace"])
        assert got == c["sample"], i
        assert rng.getrandbits(32) == c["next"], i
    assert 0 < raised < len(cases) // 4


def test_kats_reach_every_event():
    stats = {}
    for c in M.load_kats():
        LE.note_events(random.Random(c["seed"]), c["segments"], c["workspace"], stats)
    assert [e for e in EVENTS if not stats.get(e)] == []
    assert stats.get("ValueError") and stats.get("OverflowError")


def test_gpu_unit_generators_reach_every_event():
    """the units tests/test_sampler_local_permutation.py generates (random, fixed shapes, the small-piece unit), under
    the seeds it uses."""
    stats = {}
    for seed in LE.SEEDS:
        flat = LE.units_flat(LE.random_units(random.Random(seed), LE.N_RANDOM_UNITS))
        LE.model_units(flat, seed, 0, LE.N_SAMPLES, stats=stats)
    for _, units in LE.fixed_units():
        LE.model_units(LE.units_flat(units), 3, 0, 2, stats=stats)
    assert [e for e in EVENTS if not stats.get(e)] == []
