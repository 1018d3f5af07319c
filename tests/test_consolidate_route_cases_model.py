"""tests/consolidate_route_cases.py on the oracle alone (no GPU): every input is one the reference accepts, the lists are as long
as the case is about, the per-sample placed counts fall on the sides the case names -- and the module's border arithmetic agrees
with a second statement of the same rules, written here from bytes and counts instead of the code's expressions, and with the
sizes a first reading of the rules by hand gave (approximate: within two)."""
import numpy as np
import pytest

import consolidate_route_cases as K

LDS_BYTES = 163840


# ------------------------------------------------------------------------------------------------ the arithmetic, a second time
def _cap(n):
    """a unit's slab region: its segments, a quarter, 96 -- in whole blocks of 64"""
    need = n + n // 4 + 96
    return need + (-need) % 64


def _route(n):
    """(what consolidates a one-unit problem of n > 1 024 segments first, its detail), from bytes: a segment is 8 bytes, a
    histogram word 4, the generator's state 2 560; k_merge_big keeps 1 KiB back"""
    cap = _cap(n)
    if 2560 + 8 * cap > LDS_BYTES:
        return ("huge", 0)
    hist = 8192 if cap > 4096 else (4096 if cap > 2048 else (2048 if cap > 1024 else 1024))
    if 8 * cap + 4 * (hist + 1) + 1024 <= LDS_BYTES:
        expected = n + n // 12 + 64
        ccap = min(cap, expected + (-expected) % 64)
        per_thread = -(-ccap // 512)
        regs = [r for r in (8, 16, 24) if per_thread <= r]
        return ("merge_big", regs[0] if regs else 0)
    for b in (hist, hist // 2, hist // 4, hist // 8):
        if b >= 1024 and 2560 + 8 * cap + 4 * (b + 1) <= LDS_BYTES:
            return ("sampler", b)
    return ("sampler", 0)


def test_border_arithmetic_against_a_second_statement():
    routes = [_route(n) for n in range(1025, 22001)]
    change = dict()
    for k in range(1, len(routes)):
        if routes[k] != routes[k - 1]:
            change[(routes[k - 1], routes[k])] = 1025 + k - 1            # the last n of the earlier route
    B = K.borders()
    want = {"ccap4096": (("merge_big", 8), ("merge_big", 16)), "ccap8192": (("merge_big", 16), ("merge_big", 24)),
            "ccap12288": (("merge_big", 24), ("merge_big", 0)), "merge_big": (("merge_big", 0), ("sampler", 4096)),
            "big_buckets4096": (("sampler", 4096), ("sampler", 2048)), "big_buckets2048": (("sampler", 2048), ("sampler", 1024)),
            "big_buckets1024": (("sampler", 1024), ("sampler", 0)), "lds": (("sampler", 0), ("huge", 0))}
    assert len(change) == len(want) == len(B), change              # every route once, in this order: no border crossed twice
    for key, step in want.items():
        assert change[step] == B[key], (key, change[step], B[key])
    # the sizes a reading by hand gave: the borders as plain numbers, should both statements ever move together
    for key, near in (("ccap4096", 3721), ("ccap8192", 7502), ("ccap12288", 11283), ("merge_big", 12876), ("big_buckets4096", 14362),
                      ("big_buckets2048", 15180), ("big_buckets1024", 15590), ("lds", 16051)):
        assert abs(B[key] - near) <= 2, (key, B[key])
    # ... and the plan of the module on both sides of each
    for n in range(1025, 22001, 37):
        P, (kind, detail) = K.plan([n]), _route(n)
        assert P["huge"] == (kind == "huge") and P["merge_big"] == (kind == "merge_big"), n
        assert P["big_buckets"] == (detail if kind == "sampler" else 0), n
        assert P["classes"][0]["merge_form"] == (detail if kind == "merge_big" else -1), n
    # n + n / 8 reaches 1 024 at 911 (911 + 113) and passes it at 912: the last unit of the split path, the first long one
    assert [K.is_long(n) for n in (910, 911, 912)] == [False, False, True]
    assert K.plan([911])["split"] == 1 and K.plan([912])["split"] == 0 and K.plan([912])["merge_big"] == 1


def test_the_plans_cover_every_route():
    """groups b and d between them: every k_merge_big form, TREE and not, every big_buckets and huge -- and the two sides of
    every border plan differently"""
    plans = dict((name, K.expected_plan(name)) for name in K.names("b") + K.names("d"))
    forms = set((P["classes"][0]["merge_form"], P["tree"]) for P in plans.values() if P["merge_big"])
    assert set(f for f, _ in forms) == {8, 16, 24, 0} and (8, 1) in forms and (24, 1) in forms and (8, 0) in forms and (24, 0) in forms
    assert set(P["big_buckets"] for P in plans.values() if not P["merge_big"] and not P["huge"]) == {4096, 2048, 1024, 0}
    assert any(P["huge"] for P in plans.values())
    pairs = dict()
    for c in K.cases().values():
        if c.pair:
            pairs.setdefault((c.group, c.pair), []).append(c.name)
    assert len(pairs) == 8
    for key, two in pairs.items():
        assert len(two) == 2 and plans[two[0]] != plans[two[1]], key
    # the mixed problems: the short and the long units share the largest unit's route
    P = K.expected_plan("d_mixed_merge_big")
    assert P["merge_big"] == 0 and P["big_buckets"] == 4096 and P["n_long"] == 4 and P["n_classes"] == 5
    P = K.expected_plan("d_mixed_lds")
    assert P["huge"] == 1 and P["split"] == 0 and P["n_long"] == 0


# ------------------------------------------------------------------------------------------------ the cases on the oracle
@pytest.mark.parametrize("group", ["a", "b", "c", "d"])
def test_cases_are_valid_for_the_reference(group):
    for name in K.names(group):
        case = K.cases()[name]
        flat, want, (seg, off) = K.reference(name)                     # (no ValueError, no assertion of the oracle's)
        assert len(off) == case.S * int(flat["n_contigs"]) + 1 and len(want) == len(case.counters), name
        ns = K.working(case)
        assert ns == [len(s) for s, _ in case.units], name             # every segment is a working segment: n is what the case says
        P = K.expected_plan(name)
        lens = np.diff(off).reshape(case.S, -1)
        placed = np.array(K.placed_counts(name))
        assert placed.shape == (case.S, len(ns)), name
        if len(ns) == 1:
            # a final list is what the first consolidation left, a few segments more or fewer: the overlaps among the placed
            # segments (n c / 2 of them at coverage c <= 1 %) merged, and about as many placed again behind it
            if case.spread:
                assert np.all(np.abs(lens[:, 0] - placed[:, 0]) <= 0.02 * ns[0] + 8), name
        if case.verdict == "short":
            assert P["split"] == 1 and P["merge_big"] == 0 and 512 < ns[0] <= 911 and placed.max() <= P["classes"][0]["consolidate_ccap"], name
        elif P["merge_big"]:
            ccap = P["classes"][0]["merge_ccap"]
            take = K.takeable(name)
            if case.verdict == "both":
                low = placed[:, 0] <= case.straddle
                assert 0 < low.sum() < case.S, (name, int(low.sum()))
                assert case.straddle in (1024, ccap) and placed.max() <= K.cap_for(ns[0]), name    # (no slab overflow, no retry)
                assert 0 < take[0] < case.S, name
            elif case.verdict == "decline":
                assert take == [0] and placed.min() > 1024 and placed.max() <= ccap, name       # (declined for its buckets alone)
                assert K.fullest_bucket(case, 0) > 4 * K.MAX_BUCKET, name
            elif case.spread and group != "a":
                assert take == [case.S] and lens.min() > 1024, name       # every list is k_merge_big's
            if name in ("b_regs16_top", "b_regs24_top"):
                top = (placed[:, 0] > ccap - K.MERGE_THREADS) & (placed[:, 0] <= ccap)
                assert top.sum() > 0 and P["classes"][0]["merge_form"] in (16, 24), name
                assert ccap in (8192, 12288), name
        if name in ("a912", "a960"):
            assert placed.max() <= 1024, name                  # every list returns from k_merge_big at once: k_sampler's
        if name == "a1000":
            assert 0 < (placed > 1024).sum() <= 5 and K.takeable(name) == [int((placed > 1024).sum())], name   # (all but a few)
        if "direct" in name and P["merge_big"]:
            # `direct` in k_merge_big: fewer positions than the buckets the list's length asks for -- the 8 192-bucket case alone
            nbs = [K.merge_nb(int(p), P["classes"][0]["merge_buckets"]) for p in placed[:, 0]]
            if name.startswith("c_direct8192"):
                assert all(K.merge_span(case) < nb for nb in nbs) and set(nbs) == {8192}, name
                assert placed.min() > 1024 and placed.max() <= P["classes"][0]["merge_ccap"] and K.takeable(name) == [case.S], name
                assert P["classes"][0]["merge_form"] == 24, name
            else:
                assert all(K.merge_span(case) >= nb for nb in nbs), name
        if name in K.MORE_ROWS:
            assert K.base_name(name) in K.NEEDS_ROWS and K.cases()[K.base_name(name)].units == case.units, name
        if name in K.NEEDS_ROWS:
            used = K.used_outputs(name)                        # (asserts the replay gives the oracle's lists)
            assert len(used) == case.S and min(used) > 4 * ns[0], name       # several outputs per segment: rounds mostly rejected
        if case.loose:
            assert K.placed_counts(name) is K.placed_counts(K.base_name(name))
