"""GPU: more active units than one grid dimension holds, for the four samplers that run a wave per (sample, unit) and find
their unit as blockIdx.y + blockIdx.z * gridDim.y -- k_shift, k_permute, k_permute_local and k_circular.  The annotator path
(test_hip_parity.py: test_more_units_than_a_grid_dimension) and k_brute_force (test_sampler_brute_force_edges_gpu.py) have
such a test; these four did not.  66 000 units of one segment in a workspace of two short pieces, 1 sample: every unit's
coordinates are its own, so a list written for the wrong unit cannot pass.  The models take a fraction of a millisecond per
unit: the units at the borders of blockIdx.z and a stride through the rest are compared, and the length and the place of
every list."""
import pytest

import circular_cases as CIRC
import circular_model
import local_permutation_edges as LP
import local_permutation_model
import permutation_model
import sampler_edges as E
import shift_model
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, SEED = 66000, 7
BORDERS = (0, 32767, 32768, 65535, 65536, N - 1)
PICKED = sorted(set(BORDERS) | set(range(0, N, 33)))


@pytest.fixture(scope="module")
def ctx():
    from gat_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def unit(u):
    """two bases at 10 u + 1 in [10 u, 10 u + 3) + [10 u + 5, 10 u + 9); every fourth unit's segment bridges the gap"""
    return ([(10 * u + 1, 10 * u + 3)] if u % 4 else [(10 * u + 2, 10 * u + 7)]), [(10 * u, 10 * u + 3), (10 * u + 5, 10 * u + 9)]


UNITS = [unit(u) for u in range(N)]
# SamplerLocalPermutation takes a workspace piece's run of segments as a whole and, as the reference does, places it anywhere below
# the piece's end: no segment may reach beyond its piece, and a list lies below its unit's workspace end, not inside the workspace
PLAIN_UNITS = [([(10 * u + 1, 10 * u + 3)], w) for u, (_, w) in enumerate(UNITS)]


def shift(rng, segs, ws):
    return shift_model.sample(rng, segs, ws, 2.0, 0, {})


CASES = {
    "shift": (UNITS, lambda: E.units_flat(UNITS, E.SHIFT, 2.0, 0), O.RandomState, shift),
    "global-permutation": (UNITS, lambda: E.units_flat(UNITS, E.PERM), E.CountingRandom, lambda rng, s, w: permutation_model.sample(rng, s, w, {})),
    "local-permutation": (PLAIN_UNITS, lambda: LP.units_flat(PLAIN_UNITS), E.CountingRandom, local_permutation_model.sample),
    "circular": (UNITS, lambda: CIRC.units_flat(UNITS), O.RandomState, circular_model.sample),
}


def test_the_picked_units():
    assert len(PICKED) >= 2000 and all(b in PICKED for b in BORDERS) and N > 65535 + 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_more_units_than_a_grid_dimension(ctx, name):
    units, make, stream, model = CASES[name]
    flat = make()
    assert int(flat["n_units"]) == N and int((flat["unit_contig"] >= 0).sum()) == N > 65535      # every unit is active
    got, st = E.device_units(ctx, flat, SEED, 0, 1)
    assert len(got) == N
    for u in PICKED:
        want = [tuple(x) for x in model(stream((SEED + u) & 0xFFFFFFFF), *units[u])]
        assert got[u] == want, (name, u, got[u], want)
    # every unit wrote a list, and wrote it in its own workspace
    for u, g in enumerate(got):
        assert g and g[-1][1] <= 10 * u + 9 and (name == "local-permutation" or 10 * u <= g[0][0]), (name, u, g)
