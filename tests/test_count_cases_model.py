"""CPU only: the inputs of tests/count_cases.py have the properties their cases are named for, pass the library's check_list
(restated), and the per-base mask model agrees with oracle.counter wherever it applies -- before any device is asked."""
import numpy as np
import pytest

import count_cases as K

CASES = K.direct_cases()


def _agree(case):
    want = case.expected(K.COUNTERS)
    model, applies = K.model_expected(case, K.COUNTERS)
    n = 0
    for k, c in enumerate(K.COUNTERS):
        if model is None:
            assert not applies[k].any()
            continue
        ok = applies[k]
        assert np.array_equal(model[k][ok], want[k][ok]), (case.name, c)          # (density: the same double, bit for bit)
        n += int(ok.sum())
    return n, sum(a.size for a in applies)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_premise_and_lists(case):
    assert case.branch and case.premise is not None or case.name.startswith("roles_exchanged")
    for a in case.lists + case.annos:
        assert a.dtype == K.SEG and K.check_list(a) is None
    if case.premise is not None:
        case.premise(case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_equals_oracle(case):
    n, total = _agree(case)
    if case.max_coord() <= K.MODEL_MAX:
        # the four overlap counters always apply; the midpoint pair wherever no midpoint lies in a later interval
        assert n >= total * 4 // 6
    else:
        assert n == 0 and case.name in ("highest_coordinates", "sum_beyond_32_bits")


def test_roles_exchanged_is_the_same_question():
    """annotation-overlap / -midoverlap of the exchanged case ARE segment-overlap / -midoverlap of the original"""
    by_name = dict((c.name, c) for c in CASES)
    n = 0
    for name, c in by_name.items():
        if not name.startswith("roles_exchanged:"):
            continue
        o = by_name[name[len("roles_exchanged:"):]]
        a, b = c.expected(K.COUNTERS), o.expected(K.COUNTERS)
        assert np.array_equal(a[4], b[2].T) and np.array_equal(a[5], b[3].T)
        assert np.array_equal(a[2], b[4].T) and np.array_equal(a[3], b[5].T) and np.array_equal(a[0], b[0].T)
        n += 1
    assert n == 3


def test_edge_probes_hit_both_sides_of_every_comparison():
    """around [a, b): the midpoint counter says 0 at a - 1 and b, 1 at a and b - 1; the overlap counter 0 for the bases next
    to the interval and 1 for its first and last base -- an off-by-one in `mid < pe_raw`, `sk <= mid` or `pe_raw > xs` moves one"""
    case = K.edges_of_one_interval(1000, 1010)
    want = case.expected(K.COUNTERS)
    col = dict((n, i) for i, n in enumerate(case.probe_names))
    mid, ov, nuc = want[3][0], want[2][0], want[0][0]
    for length in (5, 6):
        assert mid[col["midpoint a-1, length %d" % length]] == 0 and mid[col["midpoint b, length %d" % length]] == 0
        assert mid[col["midpoint a, length %d" % length]] == 1 and mid[col["midpoint b-1, length %d" % length]] == 1
        assert all(ov[col["midpoint %s, length %d" % (w, length)]] == 1 for w in ("a-1", "a", "b-1", "b"))
    assert ov[col["last base before a"]] == 0 and ov[col["first base behind b"]] == 0
    assert ov[col["first base"]] == 1 and ov[col["last base"]] == 1
    assert ov[col["bookended at a"]] == 1 and ov[col["bookended at b"]] == 1
    assert nuc[col["one base wider"]] == 10 and nuc[col["the interval"]] == 10 and nuc[col["bookended at a"]] == 3


def test_refused_lists_are_what_check_list_refuses():
    for lists, annos, code in K.refused():
        assert code == K.ERR_ARG
        assert [K.check_list(lists), K.check_list(annos)].count(K.ERR_ARG) == 1
    assert K.check_list(K.seg([(5, 5)])) == K.ERR_ASSERT and K.check_list(K.seg([(5, 9), (8, 12)])) == K.ERR_ASSERT
    assert K.check_list(K.seg([(5, 9), (9, 12), (12, K.TOP)])) is None           # bookended, and the highest end


def test_fuzz_seeds_are_valid_and_varied():
    """all 100 seeds: valid lists, the model agrees with the oracle; and together they hold what they were drawn for"""
    gaps, staged16, unstaged16, empties, longest, slow_mid = set(), 0, 0, 0, 0, 0
    for seed in K.FUZZ_SEEDS:
        case = K.fuzz(seed)
        for a in case.lists + case.annos:
            assert K.check_list(a) is None
            if len(a) > 1:
                gaps |= set(np.unique(a["start"][1:].astype(np.int64) - a["end"][:-1]).tolist())
            empties += len(a) == 0
            longest = max(longest, len(a))
        assert case.max_coord() <= K.MODEL_MAX
        n, total = _agree(case)
        slow_mid += total - n
        c16 = K.fuzz_under(seed, "tile16")
        staged16 += c16.staged
        unstaged16 += 1 - c16.staged
    assert {0, 1, 2} <= gaps and max(gaps) >= 1000
    assert staged16 >= 10 and unstaged16 >= 10 and empties >= 10 and longest >= 300
    assert slow_mid > 0           # (some midpoints do lie in a later interval: there the oracle alone decides)


def test_grid_rule_bound():
    """the shift the rule picks never makes a cell narrower than the bound the cluster cases rely on"""
    for max_start in (0, 15, 16, 1000, 65535, 65536, K.FAR, K.TOP - 1):
        for longest in (1, 16, 17, 65, 1021):
            for gf in (1, 2, 4):
                sh, cells = K.grid_shift(max_start, longest, gf)
                assert cells <= gf * K.pow2ceil(max(16, longest)) and (sh == 0 or ((max_start >> (sh - 1)) + 1) > gf * K.pow2ceil(max(16, longest)))
                assert (1 << sh) >= K.min_cell_width(max_start, longest, gf)
