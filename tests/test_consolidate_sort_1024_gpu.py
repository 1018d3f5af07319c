"""k_consolidate's sort of 513..1 024 placed segments on the device (wave_sort_bucket_sparse<16, 1024>: the halfword
base | count << 10, the collided buckets, the fall-back to the network beyond 16 a bucket): every case of
tests/consolidate_sort_1024_cases.py -- a one-unit problem, samples [1 000, 1 070): two tiles, the second partial -- must give
the oracle's lists and counts bit for bit and the oracle's n_placed, n_draws and n_unsuccessful, with n_full_units == 0 and
n_retried == 0: no case passes because k_sampler redid a unit from its seed.  What the cases hand the sort (lengths on both
sides of 512 | 513, 576 | 577, 960 | 961 and at 1 024, fullest buckets of 2-4, 5-8, 9-16, exactly 16, exactly 17 and more, a
count of 9-16 behind a base of 1 000, equal starts with different ends) is asserted from the oracle's replay, here and -- without
a GPU -- in tests/test_consolidate_sort_1024_cases_model.py.  A fullest bucket of one element and a list of equal starts are
not among them: the sampler cannot produce either at these lengths (the case module's docstring)."""
import collections

import numpy as np
import pytest

import consolidate_route_cases as K
import consolidate_sort_1024_cases as C
from gat_amd import _lib


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _check(ctx, name):
    case = C.cases()[name]
    flat, want, (wseg, woff) = C.reference(name)
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(list(case.counters), K.SEED, C.BEGIN, C.BEGIN + C.S)
        st1, rep = P.last_stats, ctx.sampler_report()
        seg, off = P.sample(K.SEED, C.BEGIN, C.BEGIN + C.S)
        st2 = P.last_stats
    finally:
        P.close()
    for k, c in enumerate(case.counters):
        assert np.array_equal(got[k], want[k]), (name, c)
    assert np.array_equal(off, woff) and np.array_equal(seg, wseg), name
    assert rep["split"] == 1 and rep["merge_big"] == 0 and rep["huge"] == 0, rep
    placed, draws, nuns = C.stream_stats(name)
    lengths = collections.Counter(len(lst) for lst in C.first_lists(name))
    print("%s: lists of %d..%d at the first consolidation (ccap %d), n_placed %d n_draws %d n_unsuccessful %d, queued %d of %d"
          % (name, min(lengths), max(lengths), rep["classes"][0]["consolidate_ccap"], placed, draws, nuns, st1["n_queued_units"], C.S))
    assert max(lengths) <= rep["classes"][0]["consolidate_ccap"], name
    for st in (st1, st2):
        assert st["n_full_units"] == 0 and st["n_retried"] == 0, (name, st)
        assert (st["n_placed"], st["n_draws"], st["n_unsuccessful"]) == (placed, draws, nuns), (name, st)
        assert st["n_tail_units"] + st["n_queued_units"] == C.S, (name, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in C.cases() if n.startswith("s_")])
def test_size_borders(ctx, name):
    lengths = collections.Counter(len(lst) for lst in C.first_lists(name))
    if name.startswith("s_spread"):
        assert min(lengths) <= 512 and max(lengths) >= 513, name
    if name == "s_576":
        assert lengths[576] > 0 and lengths[577] > 0
    if name == "s_960":
        assert lengths[960] > 0 and lengths[961] > 0
    if name == "s_911":
        assert K.working(C.cases()[name]) == [911]
    if name == "s_1024":
        assert lengths[1024] > 0 and lengths[1023] > 0 and lengths[1025] > 0       # exactly 1 024 occurs
    _check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in C.cases() if n.startswith("o_")])
def test_occupancy_bands(ctx, name):
    seen = collections.Counter()
    for other in C.cases():
        for o in C.occupancy(other):
            if o is not None and 512 < o.n <= 1024:
                seen[C.band_of(o.fullest)] += 1
    assert all(seen[b] >= 5 for b in C.BANDS), seen
    if name == "o_last16":                                                          # the two sides of the fall-back's border
        fullest = collections.Counter(o.fullest for o in C.occupancy(name) if o is not None and 512 < o.n <= 1024)
        assert fullest[16] > 0 and fullest[17] > 0, fullest
    _check(ctx, name)


@pytest.mark.gpu
def test_the_largest_base_meets_a_large_count(ctx):
    hits = [o for o in C.occupancy("b_base1000")
            if o is not None and o.n <= 1024 and o.last_base >= 1000 and 9 <= o.last_count <= 16 and o.fullest <= 16]
    assert len(hits) >= 5
    _check(ctx, "b_base1000")


@pytest.mark.gpu
def test_ties(ctx):
    occ = [o for o in C.occupancy("t_ties") if o is not None and 512 < o.n <= 1024]
    assert len(occ) >= C.S // 2 and all(o.ties >= 5 for o in occ)
    _check(ctx, "t_ties")
