"""The first consolidation of lists from 513 segments to beyond LDS on the device: every case of tests/consolidate_route_cases.py
(the borders of k_consolidate's and k_merge_big's forms, k_merge_big's bail-outs, the problem-wide LDS gates) must give the
oracle's counts and lists bit for bit, must have been PLANNED as the rules say (gat_sampler_last_launch against the module's
plan(): flags, form, capacity and buckets per size class, big_buckets, k_sampler's variant), and must account for its units:

  n_full_units == 0                      the front end ran: nothing was sampled from scratch by k_sampler.  The one exception
                                         is what tests/test_rows_run_out_gpu.py pins: k_tail_big and k_resume_big hold no
                                         generator, a unit whose pre-generated rows end THERE is redone from its seed.  Only the
                                         dense cases K.NEEDS_ROWS get there (half or all of their workspace covered: every
                                         stream draws several times its rows); for them, with `need` the streams whose outputs
                                         by the oracle's generator (K.used_outputs) exceed Problem.rows_per_sample():
                                         n_full_units <= need and <= n_tail_units (only a carried unit is redone), and
                                         need <= n_full_units + n_resumed_units (every such stream was switched or redone).
                                         The same problems with rows for every stream (K.MORE_ROWS): 0 again, none resumed,
                                         all carried -- there the lists come from what k_merge_big sorted
  split path (n <= 911)                  n_tail_units + n_queued_units == every (sample, unit), as tests/test_consolidate_sort.py
                                         has it; spread lists: some finished by k_tail, at most MAX_QUEUED left to k_sampler
                                         (the derivation there: a fifth new segment, a touch, a long trim -- a few per cent)
  k_merge_big .. k_queue_rest            n_tail_units counts what k_tail_big carried on (only lists k_merge_big consolidated:
                                         1 024 < placed <= ccap, takeable() from the oracle's generator), n_queued_units what
                                         k_resume_big did not finish -- a carried unit it hands back is in both, so
                                         n_tail_units <= takeable, n_queued_units >= the rest, and the two cover every unit.
                                         Spread lists with a takeable sample: some carried.  Declined cases: none carried, all queued
  no queue (merge_big off, or huge)      both are 0: k_sampler is launched over every unit

No cap on what k_resume_big hands back, and none for crowded lists (tests/test_consolidate_sort.py says why): those lists
are k_sampler's by design.  The two sides of a border must report different plans, or the border is no longer where the
case sits.  Each case prints its report (pytest -s); profiles/consolidate_route_reports.txt is such a run's output."""
import json

import numpy as np
import pytest

import consolidate_route_cases as K
from gat_amd import _lib


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


_RESULTS = {}


def _run(ctx, name):
    """the case's two calls (sample_and_count, sample) and what the context reported after each: once per case"""
    if name in _RESULTS:
        return _RESULTS[name]
    case = K.cases()[name]
    flat = K.reference(name)[0]
    if case.loose:
        ctx.options["GAT_MERGED_MIN_TRACKS"] = "1"
    if name in K.MORE_ROWS:
        ctx.options["GAT_RNG_SLACK"] = K.MORE_ROWS[name]
    try:
        P = _lib.Problem(ctx, flat)
        try:
            got = P.sample_and_count(list(case.counters), K.SEED, 0, case.S)
            first = (P.last_stats, ctx.sampler_report(), ctx.count_report())
            seg, off = P.sample(K.SEED, 0, case.S)
            second = (P.last_stats, ctx.sampler_report(), P.rows_per_sample())
        finally:
            P.close()
    finally:
        ctx.options.pop("GAT_MERGED_MIN_TRACKS", None)
        ctx.options.pop("GAT_RNG_SLACK", None)
    print("REPORT %s n=%s S=%d %s" % (name, K.working(case), case.S, json.dumps(first[1], sort_keys=True)))
    _RESULTS[name] = (got, seg, off, first, second)
    return _RESULTS[name]


def _check(ctx, name):
    case = K.cases()[name]
    _, want, (wseg, woff) = K.reference(name)
    got, seg, off, first, second = _run(ctx, name)
    for k, c in enumerate(case.counters):
        assert np.array_equal(got[k], want[k]), (name, c)
    assert np.array_equal(off, woff) and np.array_equal(seg, wseg), name
    # ---- the plan
    plan = dict(K.expected_plan(name))
    virtual = []
    for _, rep in (first[:2], second[:2]):
        rep = dict(rep)
        virtual.append(rep.pop("resume_virtual"))
        assert rep == plan, (name, rep, plan)
    # (counts through the merged index alone leave k_resume_big's log behind the list; lists somebody reads are compacted)
    assert virtual == [int(case.loose and plan["resume_big"] and not case.iso), 0], (name, virtual)
    if case.loose:
        assert _lib.COUNT_KERNELS[first[2]["kernel"]] == "k_count_merged", name
    # ---- the units
    total = case.S * len(case.units)
    take = K.takeable(name)
    for s in (first[0], second[0]):
        print("%s: n_tail_units %d, n_queued_units %d of %d, n_full_units %d, n_resumed_units %d, takeable %s"
              % (name, s["n_tail_units"], s["n_queued_units"], total, s["n_full_units"], s["n_resumed_units"], take))
        assert s["n_retried"] == 0, name                       # (no slab overflow: the plan is the first and only one)
        tail, queued = s["n_tail_units"], s["n_queued_units"]
        if name in K.NEEDS_ROWS:
            need = sum(1 for u in K.used_outputs(name) if u > second[2])
            print("%s: rows %d, %d of %d streams need more" % (name, second[2], need, total))
            assert s["n_full_units"] <= min(need, tail) and need <= s["n_full_units"] + s["n_resumed_units"], (name, need)
        else:
            assert s["n_full_units"] == 0, name
        if name in K.MORE_ROWS:
            # rows for every stream: nothing switched, nothing redone -- the lists compared above come from k_merge_big's
            assert s["n_resumed_units"] == 0 and max(K.used_outputs(name)) <= second[2] and tail == total, (name, second[2])
        if plan["split"]:
            assert tail + queued == total, name
            if case.spread:
                assert tail > 0 and queued <= K.MAX_QUEUED * total, (name, queued)
        elif plan["long_queue"]:
            takeable = sum(take)
            assert tail <= takeable and total - takeable <= queued <= total and tail + queued >= total, (name, tail, queued, takeable)
            if case.spread and takeable > 0:
                assert tail > 0, name
        else:
            assert tail == 0 and queued == 0, (name, tail, queued)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.names("a"))
def test_513_to_1024(ctx, name):
    _check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.names("b"))
def test_merge_big_forms(ctx, name):
    _check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.names("c"))
def test_merge_big_bail_outs(ctx, name):
    _check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.names("d"))
def test_lds_gates(ctx, name):
    _check(ctx, name)


@pytest.mark.gpu
def test_report_of_the_other_samplers(ctx):
    """the samplers that run one kernel per unit report no plan (variant -1, everything else 0) -- also right behind a call
    that had one --, SamplerSegments reports its k_sampler variant and neither split path nor k_merge_big"""
    import sampler_edges as E
    _run(ctx, "a520")
    units = [K.cases()["a520"].units[0]]
    for sampler, variant in ((_lib.SAMPLER_SHIFT, -1), (_lib.SAMPLER_GLOBAL_PERMUTATION, -1), (_lib.SAMPLER_SEGMENTS, 4)):
        flat = E.units_flat(units, sampler, 1.0, 0)
        flat.update(bucket_size=1, nbuckets=K.NBUCKETS)
        got, _ = E.device_units(ctx, flat, 5, 0, 2)
        assert len(got) == 2
        rep = ctx.sampler_report()
        assert rep.pop("sampler_variant") == variant, (sampler, rep)
        if variant < 0:
            assert rep.pop("classes") == [] and set(rep.values()) == {0}, (sampler, rep)
        else:
            assert (rep["split"], rep["merge_big"], rep["huge"], rep["n_classes"]) == (0, 0, 0, 1), rep


@pytest.mark.gpu
def test_the_two_sides_of_a_border_report_different_plans(ctx):
    pairs = dict()
    for c in K.cases().values():
        if c.pair:
            pairs.setdefault((c.group, c.pair), []).append(c.name)
    assert len(pairs) == 8
    for key, (near, far) in sorted(pairs.items()):
        a, b = _run(ctx, near)[3][1], _run(ctx, far)[3][1]
        assert a != b, (key, a)
