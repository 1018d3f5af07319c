"""CPU: tests/permutation_model.py (SamplerGlobalPermutation in closed form on random.Random) == the reference's own
SamplerGlobalPermutation on the known-answer cases of tests/golden/permutation/kat.json -- the sampled list and what the
sample consumed of the stream."""
import random

import permutation_model as M


def test_model_matches_reference_kats():
    cases = M.load_kats()
    assert len(cases) >= 500
    empty = wrapped = 0
    for i, c in enumerate(cases):
        rng = random.Random(c["seed"])
        got = M.sample(rng, c["segments"], c["workspace"])
        assert got == c["sample"], i
        assert rng.getrandbits(32) == c["next"], i
        empty += not got
        wrapped += any(b[0] < a[0] for a, b in zip(got, got[1:]))
    assert empty > 0 and wrapped == 0


def test_model_covers_the_edge_shapes():
    """free = 0 and free + 1 a power of two occur among the known answers; samples can leave the workspace."""
    frees, outside = set(), False
    for c in M.load_kats():
        t = M.unit_tables(c["segments"], c["workspace"])
        if t is None:
            continue
        frees.add(t[2])
        ws = c["workspace"]
        outside = outside or any(not any(s < we and e > wsb for wsb, we in ws) or s < ws[0][0] or e > ws[-1][1]
                                 for s, e in c["sample"])
    assert 0 in frees and any(f > 0 and (f + 1) & f == 0 for f in frees) and outside
