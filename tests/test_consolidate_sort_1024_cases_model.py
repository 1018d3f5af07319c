"""tests/consolidate_sort_1024_cases.py on the CPU: the oracle alone must hand k_consolidate's sort of 513..1 024 segments the
lists the cases are there for -- lengths on both sides of every border, every band of bucket occupancy the sampler can produce,
the crowded last bucket behind a base of 1 000, buckets of exactly 16 and 17, equal starts with different ends -- within the
split path's plan and the class's ccap (no GPU: the replay and the plan are the module's and consolidate_route_cases')."""
import collections

import pytest

import consolidate_route_cases as K
import consolidate_sort_1024_cases as C


def _occ(name):
    return [o for o in C.occupancy(name) if o is not None]


def _lengths(name):
    return collections.Counter(len(lst) for lst in C.first_lists(name))


@pytest.mark.parametrize("name", list(C.cases()))
def test_the_split_path_takes_every_list(name):
    case = C.cases()[name]
    (n,) = K.working(case)
    plan = K.plan([n], len(case.units[0][1]), C.S)
    ccap = plan["classes"][0]["consolidate_ccap"]
    lengths = _lengths(name)
    print(name, "n", n, "ccap", ccap, "placed", min(lengths), max(lengths))
    assert plan["split"] == 1 and plan["huge"] == 0 and plan["long_lists"] == 0
    assert 64 < min(lengths) and max(lengths) <= ccap                       # never the register path, never beyond the LDS
    assert sum(c for k, c in lengths.items() if 512 < k <= 1024) > 0        # some list of every case takes the sort under test
    assert len(_occ(name)) >= C.S // 2                                       # the scale's rounding leaves most samples decided


def test_size_borders():
    for name in ("s_spread500", "s_spread520"):
        lengths = _lengths(name)
        assert min(lengths) <= 512 and max(lengths) >= 513, name
    assert _lengths("s_576")[576] > 0 and _lengths("s_576")[577] > 0
    assert _lengths("s_960")[960] > 0 and _lengths("s_960")[961] > 0
    assert K.working(C.cases()["s_911"]) == [911] and not K.is_long(911) and K.is_long(912)
    # exactly 1 024, and its neighbours on either side (1 025: wave_sort_bucket_global's)
    assert all(_lengths("s_1024")[k] > 0 for k in (1023, 1024, 1025))


def test_occupancy_bands():
    seen = collections.Counter()
    for name in C.cases():
        for o in _occ(name):
            if 512 < o.n <= 1024:
                seen[C.band_of(o.fullest)] += 1
    print(dict(seen))
    assert all(seen[b] >= 5 for b in C.BANDS), seen        # (a fullest bucket of ONE cannot be sampled: the module's docstring)


def test_the_largest_base_meets_a_large_count():
    hits = [o for o in _occ("b_base1000") if o.n <= 1024 and o.last_base >= 1000 and 9 <= o.last_count <= 16 and o.fullest <= 16]
    print([(o.n, o.last_base, o.last_count) for o in hits])
    assert len(hits) >= 5


def test_buckets_of_exactly_16_and_17():
    fullest = collections.Counter(o.fullest for o in _occ("o_last16") if 512 < o.n <= 1024)
    assert fullest[16] > 0 and fullest[17] > 0, fullest
    assert all(o.fullest >= 15 for o in _occ("o_last27"))


def test_ties():
    occ = [o for o in _occ("t_ties") if 512 < o.n <= 1024]
    assert len(occ) >= C.S // 2 and all(o.ties >= 5 for o in occ)
