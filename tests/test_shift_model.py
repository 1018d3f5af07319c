"""CPU: tests/shift_model.py (SamplerShift restated on the oracle) == the reference's own SamplerShift on the
known-answer cases of tests/golden/shift/kat.json -- the sampled list and what the sample consumed of the stream."""
import shift_model as M
from oracle import oracle as O


def test_model_matches_reference_kats():
    cases = M.load_kats()
    assert len(cases) >= 360
    empty_seen = False
    for i, c in enumerate(cases):
        rng = O.RandomState(c["seed"])
        stats = {}
        got = M.sample(rng, c["segments"], c["workspace"], c["radius"], c["extension"], stats)
        assert got == c["sample"], i
        assert rng.randint(0, 2 ** 31) == c["next"], i
        empty_seen = empty_seen or stats.get("empty_windows", 0) > 0
    assert empty_seen
