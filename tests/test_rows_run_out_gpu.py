"""GPU: streams that run out of the rows k_rng generated ahead, at row counts the test chooses (tests/rows_cases.py).

A stream that needs more outputs than its rows is continued by k_sampler from the in-LDS generator, seeded and moved up to
the outputs consumed so far (rng_switch, gat_device.h): rows / 624 + 1 twists, pos = rows % 624, the current block of 64
tempered again when rows % 64 != 0.  Here the row count of a one-unit problem is put onto a target (GAT_RNG_SLACK=0, both
sigma knobs 0, GAT_RNG_TAIL_ROWS moved in steps of 16 until Problem.rows_per_sample() equals the target -- asserted, so a
change of the budget rule cannot empty a sweep unnoticed) and the call of 70 samples from sample 3 on -- two tiles, the second
partial -- is compared with the oracle by array equality: unit-level lists, offsets, all six counters.  A stream that goes
on one output off gives other lists.  tests/test_rows_cases_model.py shows on the oracle that every stream of a sweep
needs more than the rows asked for, and where in its unit the rows end.
"""
import numpy as np
import pytest

import rows_cases as RC
from gat_amd import _lib
from test_coordinate_range_gpu import LEAN, PLACE_ROUTES

pytestmark = pytest.mark.gpu
SEGMENT_SIDE = ["nucleotide-overlap", "nucleotide-density", "segment-overlap", "segment-midoverlap"]
EXACT = {"GAT_RNG_SLACK": "0", "GAT_RNG_SIGMA_MIN": "0", "GAT_RNG_SIGMA_MAX": "0"}
ROUTES = dict(PLACE_ROUTES, no_split={"GAT_NO_SPLIT": "1"}, lean_no_split=dict(LEAN, GAT_NO_SPLIT="1"))
B0, B1 = RC.BEGIN, RC.BEGIN + RC.SAMPLES
BUDGET_FREE = ("n_placed", "n_draws", "n_unsuccessful")    # what the row budget must not change


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _create(ctx, m, case, sampler, knobs):
    for k, v in knobs.items():
        m.setitem(ctx.options, k, v)
    return _lib.Problem(ctx, RC.flat_of(case, sampler))


def _problem_at(ctx, m, case, sampler, target, knobs):
    """the case's problem with exactly `target` rows per sample: the knobs of the budget are read when a problem is created,
    and a step of 16 in GAT_RNG_TAIL_ROWS is a step of 16 in the rows -- two creations at most."""
    t = target
    for _ in range(2):
        P = _create(ctx, m, case, sampler, dict(EXACT, GAT_RNG_TAIL_ROWS=str(t), **knobs))
        rows = P.rows_per_sample()
        if rows == target:
            return P
        P.close()
        assert rows > target and (rows - target) % 16 == 0 and t - (rows - target) > 0, (case.name, target, t, rows)
        t -= rows - target
    raise AssertionError("%s: %d rows not reached (%d at GAT_RNG_TAIL_ROWS=%d)" % (case.name, target, rows, t))


def _compare(P, name, sampler, what):
    """steps 2 and 3: the call's unit-level lists and offsets, and (SamplerAnnotator) the six counters, against the oracle.
    Returns the statistics of the list call."""
    want_seg, want_off = RC.arrays(RC.lists_of(name, sampler))
    seg, off = P.sample(RC.SEED, B0, B1, unit_level=True)
    st = P.last_stats
    assert np.array_equal(off, want_off), what
    assert np.array_equal(seg, want_seg), what
    if sampler == RC.ANNOTATOR:
        want = RC.counts_of(name)
        got = P.sample_and_count(RC.COUNTERS, RC.SEED, B0, B1)
        for k, c in enumerate(RC.COUNTERS):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, c)
        for key in BUDGET_FREE:
            assert P.last_stats[key] == st[key], (what, key)
    return st


def _run(ctx, monkeypatch, name, target, sampler=RC.ANNOTATOR, knobs=None, mixed=False, exact=False):
    """the case's call under exactly `target` rows and the knobs, against the oracle.  Every stream runs out (mixed: some do,
    some do not).  exact: the rows are GAT_RNG_TAIL_ROWS itself -- the first creation must give them."""
    case = RC.cases()[name]
    with monkeypatch.context() as m:
        if exact:
            kn = dict(EXACT, GAT_RNG_TAIL_ROWS=str(target))
            kn.update(knobs or {})
            P = _create(ctx, m, case, sampler, kn)
        else:
            P = _problem_at(ctx, m, case, sampler, target, knobs or {})
        try:
            rows = P.rows_per_sample()
            assert rows == target, (name, target, rows)
            more = RC.need_more(name, rows, sampler)
            assert (0 < more < RC.SAMPLES) if mixed else (rows < RC.min_used(name, sampler) and more == RC.SAMPLES), (name, rows)
            st = _compare(P, name, sampler, (name, sampler, target, knobs))
        finally:
            P.close()
    # the budget changes where a stream's outputs come from, never how many it takes or what is placed
    streams = RC.streams_of(name, sampler)
    assert st["n_draws"] == sum(s.used for s in streams), (name, target, knobs)
    assert st["n_placed"] == sum(s.placed for s in streams), (name, target, knobs)
    assert st["n_unsuccessful"] == sum(s.nuns for s in streams), (name, target, knobs)
    return st


def _all_resumed(st, what):
    assert st["n_resumed_units"] == RC.SAMPLES and st["n_full_units"] == 0, (what, st)


@pytest.mark.parametrize("group", range(len(RC.RESIDUE_GROUPS)))
def test_every_switch_position(ctx, monkeypatch, group):
    """mid at every value of rows % 624 (pos = 0, the partial last block 576..608, rows % 64 zero and not): every stream is
    resumed with the generator moved up, none redone from its seed"""
    for rows in RC.RESIDUE_GROUPS[group]:
        _all_resumed(_run(ctx, monkeypatch, "mid", rows), rows)


@pytest.mark.parametrize("group", range(len(RC.BLOCK_GROUPS)))
def test_block_counts(ctx, monkeypatch, group):
    """large at rows / 624 = 1, 2, 3: two to four twists.  Every stream switches in front of its first consolidation, whose
    list has 513..1024 segments (tests/test_rows_cases_model.py): the first sort after the switch is of that class.  It is
    NOT the counting sort of gat_kernels.h's `n > 512 && n <= 1024 && n == pre.x` branch: that branch lends the generator's
    624 words to the sort and its condition holds `rng.use_pre`, which is false after a switch, and `pre_len >= 0`, while a
    lane that ran out while placing hands over -3 -- after a switch such a list goes to wave_sort_fast without scratch."""
    for rows in RC.BLOCK_GROUPS[group]:
        assert all(s.first_at > rows and 513 <= s.first_n <= 1024 for s in RC.streams_of("large"))
        _all_resumed(_run(ctx, monkeypatch, "large", rows), rows)


@pytest.mark.parametrize("name", ["small", "small_b3"])
def test_small_rows(ctx, monkeypatch, name):
    """at most 65 working segments: rows == GAT_RNG_TAIL_ROWS rounded up to 16, outright; lists of at most 64 (the insertion
    sort); bucket 3 adds the draw inside the bucket"""
    for rows in RC.SMALL_ROWS:
        _all_resumed(_run(ctx, monkeypatch, name, rows, exact=True), (name, rows))
    _all_resumed(_run(ctx, monkeypatch, name, 48, knobs={"GAT_RNG_TAIL_ROWS": "33"}, exact=True), name)   # (rounded up)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["mid", "mid_simple"])
def test_routes(ctx, monkeypatch, name, route):
    """the hand-over from every placement kernel: mid (three pieces: k_place's general form) and mid_simple (one piece: by
    default a call of two tiles takes k_place_scan; under PLACE_ROUTES k_place_wide, k_place_pipe and k_place, each with the
    step written out by hand -- whose `used` is folded by GAT_FOLD_USED -- and with the compiler's), and GAT_NO_SPLIT, at
    three row counts deep in placement (the lane hands over -3) and three just under the shortest stream (the rows end
    behind the first consolidation: in k_tail, which leaves the unit to k_sampler, or between two consolidations)"""
    for rows in RC.ROUTE_ROWS_DEEP + RC.ROUTE_ROWS_LATE[name]:
        _all_resumed(_run(ctx, monkeypatch, name, rows, knobs=ROUTES[route]), (name, route, rows))


@pytest.mark.parametrize("knobs", [{}, {"GAT_PLACE_NO_GRID": "1"}, {"GAT_TAIL_NO_LONG_WS": "1"}], ids=lambda k: "-".join(k) or "default")
def test_grid_route(ctx, monkeypatch, knobs):
    """300 workspace pieces: k_place_grid hands over (GAT_PLACE_NO_GRID: k_place over the trees)"""
    for rows in (RC.SHORT_ROWS["mid_grid"], RC.MAX_ROWS["mid_grid"]):
        _all_resumed(_run(ctx, monkeypatch, "mid_grid", rows, knobs=knobs), (knobs, rows))


def test_mixed_tile(ctx, monkeypatch):
    """about half of mid's streams need more than the rows: lanes that run out and lanes that do not share a tile and a
    k_tail wave.  The resumed units are exactly the streams that need more outputs than the rows hold, by the device's
    count (the reference's last, discarded placement is not drawn)"""
    st = _run(ctx, monkeypatch, "mid", RC.MIXED_ROWS, mixed=True)
    assert 0 < st["n_resumed_units"] < RC.SAMPLES and st["n_full_units"] == 0, st
    assert st["n_resumed_units"] == RC.need_more("mid", RC.MIXED_ROWS), st


@pytest.mark.parametrize("knobs", [{}, {"GAT_NO_RESUME_BIG": "1"}, {"GAT_NO_TAIL_BIG": "1"}], ids=lambda k: "-".join(k) or "default")
def test_long_lists(ctx, monkeypatch, knobs):
    """lists beyond 1024.  A short budget: every lane hands over -3 and k_sampler switches.  A late one: k_tail_big and
    k_resume_big have no LDS for a generator -- a unit whose rows end there is marked (state 3) and redone from its seed"""
    st = _run(ctx, monkeypatch, "long", RC.SHORT_ROWS["long"], knobs=knobs, exact=True)
    assert st["n_resumed_units"] + st["n_full_units"] == RC.SAMPLES, st
    st = _run(ctx, monkeypatch, "long", RC.LONG_LATE_ROWS, knobs=knobs, mixed=True, exact=True)
    assert RC.need_more("long", RC.LONG_LATE_ROWS) <= st["n_resumed_units"] + st["n_full_units"] < RC.SAMPLES, st
    if not knobs:
        assert st["n_full_units"] > 0, st


@pytest.mark.parametrize("name", ["small", "mid"])
def test_segments_are_redone_from_the_seed(ctx, monkeypatch, name):
    """SamplerSegments hands over -1: no switch, every unit is run in full from its seed"""
    for knobs in ({}, LEAN):
        st = _run(ctx, monkeypatch, name, RC.SHORT_ROWS[name], sampler=RC.SEGMENTS, knobs=knobs, exact=True)
        assert st["n_full_units"] == RC.SAMPLES and st["n_resumed_units"] == 0, (name, knobs, st)


def _counts_alone(P, name, what):
    """a fresh problem's first calls are counts: the segment-side counters (merged lists + k_tail's records where the
    library reads those), then all six"""
    want = RC.counts_of(name)
    seen = []
    for sub in (SEGMENT_SIDE, RC.COUNTERS):
        got = P.sample_and_count(sub, RC.SEED, B0, B1)
        seen.append(dict(P.last_stats))
        for k, c in enumerate(sub):
            assert got[k].dtype == want[RC.COUNTERS.index(c)].dtype and np.array_equal(got[k], want[RC.COUNTERS.index(c)]), (what, c)
    return seen


@pytest.mark.parametrize("name", ["mid", "multi"])
def test_counts_alone(ctx, monkeypatch, name):
    """counts without lists under a shortage: the units k_sampler resumed arrive in the form k_count_seg / k_contig read
    (lists_from_records where the default budget has it too)"""
    case = RC.cases()[name]
    with monkeypatch.context() as m:
        P = _create(ctx, m, case, RC.ANNOTATOR, {})
        try:
            default = _counts_alone(P, name, (name, "default"))
        finally:
            P.close()
    with monkeypatch.context() as m:
        if name == "multi":
            P = _create(ctx, m, case, RC.ANNOTATOR, {"GAT_RNG_SLACK": "0.6"})
        else:
            P = _problem_at(ctx, m, case, RC.ANNOTATOR, RC.SHORT_ROWS[name], {})
        try:
            short = _counts_alone(P, name, (name, "short"))
        finally:
            P.close()
    for d, s in zip(default, short):
        assert s["n_resumed_units"] > 0 and s["n_full_units"] == 0, s
        assert (s["lists_from_records"] != 0) == (d["lists_from_records"] != 0), (d, s)
        for key in BUDGET_FREE:
            assert s[key] == d[key], (name, key)
    assert default[0]["lists_from_records"] != 0           # (the segment-side counters of a split-path problem)


@pytest.mark.parametrize("slack", ["0.3", "0.6", "0.9"])
def test_multi_under_slack(ctx, monkeypatch, slack):
    """four units of different size classes, two of them the isochores of one contig, with 0.3 / 0.6 / 0.9 of the expected
    outputs and the usual spread and tail terms: unit-level and contig-level lists and all six counters"""
    case = RC.cases()["multi"]
    lists = RC.lists_of("multi")
    with monkeypatch.context() as m:
        P = _create(ctx, m, case, RC.ANNOTATOR, {"GAT_RNG_SLACK": slack})
        try:
            st = _compare(P, "multi", RC.ANNOTATOR, ("multi", slack))
            want_seg, want_off = RC.arrays(RC.contig_lists(case, lists))
            seg, off = P.sample(RC.SEED, B0, B1)
            assert np.array_equal(off, want_off) and np.array_equal(seg, want_seg), slack
            assert P.last_stats["n_resumed_units"] > 0, P.last_stats
        finally:
            P.close()
    assert st["n_resumed_units"] > 0 and st["n_full_units"] == 0, st
    assert st["n_draws"] == sum(s.used for s in RC.streams_of("multi")), slack


@pytest.mark.parametrize("name", list(RC.cases()))
def test_statistics_do_not_depend_on_the_budget(ctx, monkeypatch, name):
    """n_placed, n_draws and n_unsuccessful of the default budget equal the oracle's -- n_draws: the oracle's D less the
    last, discarded placement of every stream (`used`) -- and a short budget reports the same three: it may change only
    n_resumed_units, n_full_units, n_retried and the split between k_tail and the queue"""
    case = RC.cases()[name]
    streams = RC.streams_of(name)
    want = dict(n_draws=sum(s.used for s in streams), n_placed=sum(s.placed for s in streams),
                n_unsuccessful=sum(s.nuns for s in streams))
    assert want["n_draws"] < sum(s.D for s in streams)
    with monkeypatch.context() as m:
        P = _create(ctx, m, case, RC.ANNOTATOR, {})
        try:
            default = _compare(P, name, RC.ANNOTATOR, (name, "default"))
        finally:
            P.close()
    with monkeypatch.context() as m:
        if name == "multi":
            P = _create(ctx, m, case, RC.ANNOTATOR, {"GAT_RNG_SLACK": "0.6"})
        else:
            P = _problem_at(ctx, m, case, RC.ANNOTATOR, RC.SHORT_ROWS[name], {})
        try:
            short = _compare(P, name, RC.ANNOTATOR, (name, "short"))
        finally:
            P.close()
    print(name, {k: (default[k], short[k]) for k in default if k.startswith("n_") and (default[k] or short[k])})
    for key in BUDGET_FREE:
        assert default[key] == want[key], (name, key, default[key], want[key])
        assert short[key] == default[key], (name, key, short[key], default[key])
    assert short["n_resumed_units"] + short["n_full_units"] > default["n_resumed_units"] + default["n_full_units"], (default, short)
