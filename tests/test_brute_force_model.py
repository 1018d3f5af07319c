"""CPU: tests/brute_force_model.py (SamplerBruteForce on the oracle's RandomState) == the reference's own SamplerBruteForce
on the known-answer cases of tests/golden/brute_force/kat.json -- the sampled list and the next draw of the stream, or the
exception the reference raised."""
import pytest

from oracle import oracle as O

import brute_force_model as M


def _run(c, stats=None):
    rng = O.RandomState(c["seed"])
    return M.sample(rng, c["segments"], c["workspace"], stats=stats, **c["params"]), rng


def test_model_matches_reference_kats():
    cases = M.load_kats()
    compared = raised = 0
    for i, c in enumerate(cases):
        if c["error"]:
            with pytest.raises(ValueError) as e:
                _run(c)
            assert type(e.value).__name__ == c["error"], i
            raised += 1
            continue
        got, rng = _run(c)
        assert got == c["sample"], i
        assert rng.randint(0, 2 ** 31) == c["next"], i
        compared += 1
    assert compared >= 250 and raised > 0


def test_random_kats_are_not_made_of_failures():
    rnd = [c for c in M.load_kats() if c["kind"] == "random"]
    assert len(rnd) >= 300
    failed = sum(1 for c in rnd if c["error"])
    assert failed < 0.25 * len(rnd), (failed, len(rnd))
    assert sum(1 for c in rnd if not c["error"]) >= 250


def test_kats_reach_the_shapes():
    """restarts, non-convergence, lists beyond one and two wave widths, an empty working list, the largest sum a list can
    have (2^31 - 996: the reference's list constructor keeps no coordinate beyond 2^31 - 1)"""
    stats = {}
    lengths = []
    big = 0
    for c in M.load_kats():
        big = max(big, sum(e - s for s, e in c["segments"]))
        try:
            got, _ = _run(c, stats)
        except ValueError:
            continue
        lengths.append(len(got))
    assert stats["restarts"] > 0 and stats["unconverged"] > 0 and stats["tries"] > 0
    assert any(64 < n <= 128 for n in lengths) and any(n > 128 for n in lengths) and 0 in lengths
    assert big == 2 ** 31 - 996
