"""GPU: the samplers that draw lengths at both ends of the coordinate range (tests/range_cases.py), on every kernel route.
Every comparison is array equality with the oracle -- the sampled (sample, unit) lists, their offsets and all six counters --
or with the reference's own lists (tests/golden/coordinate_range.json); tests/test_range_cases_model.py shows on the oracle
that each case reaches the edge it is named for.  One base past the border gat_problem_create refuses, before any kernel."""
import numpy as np
import pytest

import range_cases as R
from gat_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu
T = R.T
SEGMENT_SIDE = ["nucleotide-overlap", "nucleotide-density", "segment-overlap", "segment-midoverlap"]
# the placement kernels of a small call, from the library's own pick down to the lean kernels: k_place_scan (simple units) or
# k_place's general form -> k_place_wide -> k_place_pipe -> k_place, each with the step written out by hand and with the
# compiler's (GAT_PLACE_NO_CM)
LEAN = {"GAT_PLACE_SCAN_TILES": "0", "GAT_PLACE_NO_WIDE": "1"}
PLACE_ROUTES = {
    "default": {},
    "no_cm": {"GAT_PLACE_NO_CM": "1"},
    "no_pipe": {"GAT_PLACE_NO_PIPE": "1"},
    "wide": {"GAT_PLACE_SCAN_TILES": "0"},
    "lean": LEAN,
    "lean_no_cm": dict(LEAN, GAT_PLACE_NO_CM="1"),
    "lean_no_pipe": dict(LEAN, GAT_PLACE_NO_PIPE="1"),
    "lean_no_pipe_no_cm": dict(LEAN, GAT_PLACE_NO_PIPE="1", GAT_PLACE_NO_CM="1"),
}
SMALL = ["top_tiny_b1", "bottom", "wide_span"]
SIMPLE = ["top_simple_3000", "top_simple_2040"]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _arrays(lists):
    """(segments, offsets) of (sample, unit) lists as gat_sample_units returns them."""
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return O.segs([x for l in lists for x in l]), off


def _problem(ctx, monkeypatch, case, sampler, knobs):
    for k, v in knobs.items():
        monkeypatch.setitem(ctx.options, k, v)
    return _lib.Problem(ctx, R.flat_of(case, sampler, with_annos=sampler != R.SEGMENTS))


def _check(ctx, monkeypatch, name, sampler=R.ANNOTATOR, knobs=None):
    """the case's call on the device under the knobs: unit-level lists and offsets, and (the lists of SamplerSegments are
    not normalized: no counters) the six counters, against the oracle.  Returns the statistics of the two calls."""
    case = R.for_sampler(R.in_domain()[name], sampler)
    want_seg, want_off = _arrays(R.oracle_of(name, sampler)[0])
    P = _problem(ctx, monkeypatch, case, sampler, knobs or {})
    try:
        seg, off = P.sample(case.seed, 0, case.samples, unit_level=True)
        st_lists = P.last_stats
        assert np.array_equal(off, want_off), (name, sampler, knobs)
        assert np.array_equal(seg, want_seg), (name, sampler, knobs)
        st_counts = None
        if sampler != R.SEGMENTS:
            want = R.oracle_counts_of(name, sampler)
            got = P.sample_and_count(R.COUNTERS, case.seed, 0, case.samples)
            st_counts = P.last_stats
            for k, c in enumerate(R.COUNTERS):
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, sampler, knobs, c)
    finally:
        P.close()
    print(name, sampler, knobs, {k: v for k, v in st_lists.items() if k.startswith("n_") and v})
    return st_lists, st_counts


@pytest.mark.parametrize("route", list(PLACE_ROUTES))
@pytest.mark.parametrize("name", SMALL + SIMPLE + ["top_tiny_b3"])
def test_split_path(ctx, monkeypatch, name, route):
    """k_place* -> k_consolidate -> k_tail -> k_finalize: the step written out by hand and the compiler's agree at the border"""
    st, stc = _check(ctx, monkeypatch, name, knobs=PLACE_ROUTES[route])
    # k_tail took every (sample, unit): it finished it or left it to k_sampler's queue
    assert st["n_tail_units"] + st["n_queued_units"] == R.in_domain()[name].samples and st["n_full_units"] == 0, st
    assert stc["n_tail_units"] + stc["n_queued_units"] > 0 and stc["n_full_units"] == 0, stc
    if name != "bottom":                                   # (two fifths of its workspace covered: k_tail finishes none)
        assert st["n_tail_units"] > 0, st


@pytest.mark.parametrize("name", SMALL + SIMPLE)
def test_no_split(ctx, monkeypatch, name):
    """GAT_NO_SPLIT: k_sampler alone behind k_place"""
    st, stc = _check(ctx, monkeypatch, name, knobs={"GAT_NO_SPLIT": "1"})
    assert st["n_tail_units"] == 0 and st["n_queued_units"] == 0 and st["n_full_units"] == 0, st
    assert stc["n_tail_units"] == 0 and stc["n_queued_units"] == 0 and stc["lists_from_records"] == 0, stc
    _check(ctx, monkeypatch, name, knobs=dict(LEAN, GAT_NO_SPLIT="1"))


@pytest.mark.parametrize("name", SMALL + SIMPLE)
def test_wave_sampler(ctx, monkeypatch, name):
    """GAT_SAMPLER_MODE=wave: the stand-alone wave-per-unit sampler, its own generator in LDS"""
    st, _ = _check(ctx, monkeypatch, name, knobs={"GAT_SAMPLER_MODE": "wave"})
    assert st["n_full_units"] == R.in_domain()[name].samples and st["n_tail_units"] == 0 and st["n_queued_units"] == 0, st


@pytest.mark.parametrize("name", SMALL + SIMPLE)
def test_serial_stream(ctx, name):
    """k_serial: ONE stream through every (sample, unit) in the reference's order"""
    case = R.in_domain()[name]
    flat = R.flat_of(case, R.ANNOTATOR)
    want, _ = O.run_samples(flat, R.COUNTERS, 77, 0, 0, case.samples)
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count_serial(R.COUNTERS, _lib.mt19937_seed(77), case.samples)
    finally:
        P.close()
    for k, c in enumerate(R.COUNTERS):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, c)


@pytest.mark.parametrize("knobs", [{}, {"GAT_PLACE_NO_GRID": "1"}, {"GAT_TAIL_NO_LONG_WS": "1"}, {"GAT_GRID_CELL_SEGS": "16"},
                                   {"GAT_PLACE_NO_CM": "1"}], ids=lambda k: "-".join(k) or "default")
def test_frag_top(ctx, monkeypatch, knobs):
    """300 workspace pieces up to the border: k_place_grid (the cdf grid in LDS), the position grid in k_consolidate / k_tail,
    or the trees those replaced"""
    st, _ = _check(ctx, monkeypatch, "frag_top", knobs=knobs)
    # k_tail takes the units of a workspace of 300 pieces (and hands them all on: their streams run out of rows) unless told not to
    assert st["n_tail_units"] + st["n_queued_units"] == (0 if "GAT_TAIL_NO_LONG_WS" in knobs else 64) and st["n_resumed_units"] > 0, st
    _check(ctx, monkeypatch, "frag_top", R.SEGMENTS, knobs=knobs)


@pytest.mark.parametrize("knobs", [{}, {"GAT_NO_TAIL_BIG": "1"}, {"GAT_NO_RESUME_BIG": "1"}, {"GAT_NO_MERGE_BIG": "1"}],
                         ids=lambda k: "-".join(k) or "default")
def test_long_list_top(ctx, monkeypatch, knobs):
    """lists of 1 100 segments under the border: k_merge_big, k_tail_big, k_resume_big, and k_sampler in their place"""
    st, _ = _check(ctx, monkeypatch, "long_list_top", knobs=knobs)
    if not knobs:                                          # k_tail_big carried every unit through its placement rounds, k_resume_big
        assert st["n_tail_units"] == 64 and st["n_queued_units"] > 0, st                      # left some to k_sampler's queue
    if "GAT_NO_RESUME_BIG" in knobs:
        assert st["n_tail_units"] == 64 and st["n_queued_units"] == 0, st
    if "GAT_NO_TAIL_BIG" in knobs or "GAT_NO_MERGE_BIG" in knobs:
        assert st["n_tail_units"] == 0 and st["n_queued_units"] == 0, st


@pytest.mark.parametrize("name", ["whole_range", "half_range"])
def test_whole_and_half_range(ctx, monkeypatch, name):
    """ws_total just below 2^31 and just above 2^30; then with fewer rows generated ahead (GAT_RNG_SLACK): streams run out
    and their units are resumed from the generator moved up to their position, or redone"""
    _check(ctx, monkeypatch, name)
    st, stc = _check(ctx, monkeypatch, name, knobs={"GAT_RNG_SLACK": "0.6"})
    assert st["n_retried"] + st["n_resumed_units"] > 0 and st["n_tail_units"] + st["n_queued_units"] == 64, st
    _check(ctx, monkeypatch, name, R.SEGMENTS, knobs={"GAT_RNG_SLACK": "0.6"})


@pytest.mark.parametrize("name", ["top_tiny_b1", "wide_span"])
def test_counts_alone(ctx, monkeypatch, name):
    """the segment-side counters alone (merged list + k_tail's record, no final lists) against the counts from final lists
    (GAT_COUNT_FINAL_LISTS) and through the contig lists (GAT_COUNT_VIA_CONTIGS): the annotation's last interval ends at T"""
    case = R.in_domain()[name]
    want = R.oracle_counts_of(name, R.ANNOTATOR)
    seen = []
    for knobs in ({}, {"GAT_COUNT_FINAL_LISTS": "1"}, {"GAT_COUNT_VIA_CONTIGS": "1"}):
        with monkeypatch.context() as m:
            P = _problem(ctx, m, case, R.ANNOTATOR, knobs)
            try:
                for sub in (SEGMENT_SIDE, ["nucleotide-overlap"], ["segment-overlap", "segment-midoverlap"]):
                    got = P.sample_and_count(sub, case.seed, 0, case.samples)
                    for k, c in enumerate(sub):
                        assert np.array_equal(got[k], want[R.COUNTERS.index(c)]), (name, knobs, c)
                seen.append(P.last_stats["lists_from_records"])
            finally:
                P.close()
    assert seen[0] != 0 and seen[1] == 0, seen              # records by default, final lists under the knob


@pytest.mark.parametrize("name,sampler", [("top_tiny_b1", R.SEGMENTS), ("top_tiny_b3", R.SEGMENTS), ("bottom", R.SEGMENTS),
                                          ("bottom_0_1", R.SEGMENTS), ("bottom_0_1", R.ANNOTATOR), ("top_simple_3000", R.SEGMENTS),
                                          ("top_simple_2040", R.SEGMENTS), ("wide_span", R.SEGMENTS), ("top_tiny_b1", R.BRUTE),
                                          ("top_tiny_b3", R.BRUTE), ("bottom_brute", R.BRUTE)])
def test_segments_and_brute_force(ctx, monkeypatch, name, sampler):
    _check(ctx, monkeypatch, name, sampler)
    if sampler == R.SEGMENTS:
        _check(ctx, monkeypatch, name, sampler, knobs=LEAN)
        _check(ctx, monkeypatch, name, sampler, knobs={"GAT_SAMPLER_MODE": "wave"})


def test_the_references_own_lists(ctx):
    """tests/golden/coordinate_range.json: stream `seed` of a one-unit problem is sample `seed` of a call under seed 0"""
    n = at_T = 0
    for g in R.load_golden()["in_domain"]:
        case = R.in_domain()[g["case"]]
        assert [[list(x) for x in case.units[0][0]], [list(x) for x in case.units[0][1]]] == [g["segments"], g["workspace"]]
        streams = g["streams"]
        assert [s[0] for s in streams] == list(range(len(streams)))
        want_seg, want_off = _arrays([list(zip(flat[0::2], flat[1::2])) for _, flat, _ in streams])
        P = _lib.Problem(ctx, R.flat_of(case, g["sampler"], with_annos=False))
        try:
            seg, off = P.sample(0, 0, len(streams), unit_level=True)
        finally:
            P.close()
        assert np.array_equal(off, want_off) and np.array_equal(seg, want_seg), (g["case"], g["sampler"])
        n += len(streams)
        at_T += int((seg["end"] == T).sum())
    assert n >= 400 and at_T >= 6


@pytest.mark.parametrize("sampler", [R.ANNOTATOR, R.SEGMENTS, R.BRUTE])
def test_past_the_border_is_refused(ctx, sampler):
    """every past_border problem fails at creation with ValueError (GAT_ERR_ARG) naming the unit, the workspace end and
    the limit -- no kernel runs: the context's next problem starts from zero batches; the same workspace one base lower
    creates and samples; the shift sampler has its own rules and still creates"""
    for name, case in R.past_border().items():
        flat = R.flat_of(case, sampler)
        with pytest.raises(ValueError) as e:
            _lib.Problem(ctx, flat)
        msg = str(e.value)
        assert "error -6" in msg and "unit 0" in msg and "2^31 - 1" in msg and "2147483647" in msg, (name, msg)
        assert ("workspace end %d" % case.units[0][1][-1][1]) in msg, (name, msg)
        assert ("length %d" % R.lmax_of(*case.units[0], case.bucket_size)) in msg, (name, msg)
        lower = R.moved(case, -1)
        if R.highest_end(lower) == T and not (sampler == R.BRUTE and not name.startswith(("top_tiny", "bottom_brute"))):
            P = _lib.Problem(ctx, R.flat_of(lower, sampler, with_annos=False))
            try:
                assert P.last_stats is None                # (nothing has run on it yet)
                seg, off = P.sample(lower.seed, 0, 2, unit_level=True)
                assert P.last_stats["n_batches"] >= 1 and len(seg) > 0 and int(seg["end"].max()) <= T
            finally:
                P.close()
        P = _lib.Problem(ctx, R.flat_of(case, R.SHIFT, with_annos=False))
        P.close()
    # a second unit past the border is named as such, an inactive one (no working segment) is not looked at
    ok, bad = R.in_domain()["top_tiny_b1"], R.past_border()["top_tiny_b1+1"]
    two = ok._replace(units=ok.units + bad.units, annos=None)
    with pytest.raises(ValueError, match="unit 1"):
        _lib.Problem(ctx, R.flat_of(two, sampler))
    idle = ok._replace(units=ok.units + [([(5, 9)], bad.units[0][1])], annos=None)
    P = _lib.Problem(ctx, R.flat_of(idle, sampler))
    P.close()
