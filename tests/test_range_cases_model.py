"""The cases of tests/range_cases.py on the oracle alone (no device): every case lies where it claims to lie in the
placement domain, every premise -- the edge the case exists for -- shows in the oracle's output, and the oracle equals the
reference's own lists (tests/golden/coordinate_range.json) on them.  A case that stops exercising its edge fails here."""
import bisect

import pytest

import range_cases as R
from oracle import oracle as O

T = R.T
LIST_SAMPLERS = (R.ANNOTATOR, R.SEGMENTS)
AT_BORDER = ("top_tiny_b1", "top_tiny_b3", "wide_span", "whole_range", "frag_top", "long_list_top", "top_simple_3000", "top_simple_2040")


def test_cases_lie_where_they_claim():
    """in-domain: no placement can end above T, and the border cases can end exactly at it; past_border: one base above
    (top_tiny with its last piece at (T - 1, T): three), with the very same segments and pieces otherwise."""
    cases = R.in_domain()
    for name, c in cases.items():
        assert R.highest_end(c) <= T, name
        assert (R.highest_end(c) == T) == (name in AT_BORDER), name
        for segs, ws in c.units:
            assert O.check(segs) and O.check(ws) and len(O.filter(segs, ws)) == len(segs), name       # normalized, all working
    past = R.past_border()
    assert len(past) == len(cases) + 1
    for name, c in past.items():
        want = T + 3 if name == "top_tiny_last_piece_at_T" else T + 1
        assert R.highest_end(c) == want, name
        assert max(e for _, ws in c.units for _, e in ws) <= T                                           # (coordinates themselves stay valid)
        one_lower = R.moved(c, -1)
        assert (R.highest_end(one_lower) == T) == (name != "top_tiny_last_piece_at_T")
    for name in cases:                                     # (the refusal test's "same workspace one base lower" is the in-domain case)
        moved = [p for p in past.values() if p.name.startswith(name + "+")]
        assert len(moved) == 1 and R.moved(moved[0], -int(moved[0].name.rsplit("+", 1)[1])).units == cases[name].units


def test_lmax_is_the_largest_length_the_histogram_returns():
    """lmax_of against every length HistogramSampler can return: each rank randint(1, total) can name, each draw inside
    the bucket."""
    for name, c in R.in_domain().items():
        for segs, ws in c.units:
            hist, bucket = O.length_distribution(O.aslist(O.filter(segs, ws)), c.bucket_size, R.NBUCKETS)
            assert bucket == R.bucket_of(segs, ws, c.bucket_size)
            ranks = [i for i, n in enumerate(hist) for _ in range(int(n))]           # rank r (1-based) -> bucket index
            drawable = ranks[:-1] if len(ranks) > 1 else ranks                       # randint(1, total): r < total
            assert R.lmax_of(segs, ws, c.bucket_size) == max(drawable) * bucket + (bucket - 1 if bucket > 1 else 0), name
    assert R.lmax_of(*R.whole_range().units[0], 0) > max(e - s for s, e in R.whole_range().units[0][0])     # bucket 168


@pytest.mark.parametrize("bucket_size", [1, 3])
@pytest.mark.parametrize("sampler", [R.ANNOTATOR, R.SEGMENTS, R.BRUTE])
def test_top_tiny_ends_at_T(sampler, bucket_size):
    lists, _ = R.oracle_of("top_tiny_b%d" % bucket_size, sampler)
    at, above = R.ends_at_T(lists)
    assert at > 0 and above == 0
    if bucket_size == 1 and sampler != R.BRUTE:            # (seed 0: the counts the domain was measured with)
        assert at == {R.ANNOTATOR: 2, R.SEGMENTS: 1}[sampler]
    if bucket_size == 3:                                   # a drawn length beyond every segment of the unit
        assert max(e - s for l in R.oracle_of("top_tiny_b3", R.SEGMENTS)[0] for s, e in l) == 8


@pytest.mark.parametrize("width", [3000, 2040])
@pytest.mark.parametrize("sampler", LIST_SAMPLERS)
def test_top_simple_ends_at_T(sampler, width):
    """one piece, bucket 1, fewer than kPlaceRankLds segments: what gat_prep.hip calls a simple unit; the offset draw's range
    c + length crosses a power of two (2048) only under width 2040"""
    (segs, ws), = R.top_simple(width).units
    assert len(ws) == 1 and ws[0][1] - ws[0][0] == width and ws[0][1] == R.border(40)
    crosses = [p for p in (2048, 4096) if width < p <= width + 41]
    assert bool(crosses) == (width == 2040)
    at, above = R.ends_at_T(R.oracle_of("top_simple_%d" % width, sampler)[0])
    assert at > 0 and above == 0


@pytest.mark.parametrize("name,sampler", [("bottom", R.ANNOTATOR), ("bottom", R.SEGMENTS), ("bottom_0_1", R.ANNOTATOR),
                                          ("bottom_0_1", R.SEGMENTS), ("bottom_brute", R.BRUTE)])
def test_bottom_starts_at_0(name, sampler):
    """a start of 0 is the clamp of q <= 0: no piece of these workspaces but (0, 1) holds base 0, and a placement on (0, 1)
    has q in [-89, 0]"""
    lists, _ = R.oracle_of(name, sampler)
    assert R.starts_at_0(lists) > 0
    if sampler == R.SEGMENTS:                              # (unmerged: a clamped segment is shorter than every length drawn)
        assert any(s == 0 and e - s < 90 for l in lists for s, e in l)


@pytest.mark.parametrize("sampler", LIST_SAMPLERS)
def test_wide_span_spans_the_range(sampler):
    lists, _ = R.oracle_of("wide_span", sampler)
    assert R.widest_list(lists) > 2 ** 31 - 2 ** 21
    assert all(l and max(e for _, e in l) - min(s for s, _ in l) > 2 ** 30 for l in lists)


def test_whole_and_half_range_reject_differently():
    """the draws of a placement (the position in the workspace and the offset in the piece) per placement, counted on
    SamplerSegments, whose number of placements is fixed: about 2 under ws_total just below 2^31 (mask 0x7fffffff, almost
    no rejection), about 4 just above 2^30 (every second draw rejected) -- more than 1.5 times as many.  The length
    step's draws are the same in both (the same segments: 2.6 per placement) and are left out of the ratio; with them it
    is 6.6 : 4.6."""
    n_w, len_w, place_w = R.segments_step_draws(R.whole_range())
    n_h, len_h, place_h = R.segments_step_draws(R.half_range())
    assert n_w == n_h == 30 * 64
    assert place_h / n_h > 1.5 * place_w / n_w
    assert place_w / n_w < 2.1 and place_h / n_h > 3.5
    assert abs(len_w - len_h) < 0.05 * len_w
    for name in ("whole_range", "half_range"):             # ... and the annotator's streams show it too
        assert R.oracle_of(name, R.ANNOTATOR)[1] > 0
    assert R.oracle_of("half_range", R.ANNOTATOR)[1] > 1.3 * R.oracle_of("whole_range", R.ANNOTATOR)[1]
    segs, ws = R.whole_range().units[0]
    assert R.bucket_of(segs, ws, 0) == 168 and 2 ** 31 - 2 ** 25 < ws[0][1] - ws[0][0] < 2 ** 31
    assert R.half_range().units[0][1] == [(3, 2 ** 30 + 5)]


def test_frag_top_segments_span_pieces():
    segs, ws = R.frag_top().units[0]
    assert len(ws) > 256 and ws[-1][1] == R.border(130)
    starts = [s for s, _ in ws]
    lists, _ = R.oracle_of("frag_top", R.SEGMENTS)
    ends = [e for _, e in ws]
    spans = [bisect.bisect_left(starts, e) - bisect.bisect_right(ends, s) for l in lists for s, e in l]      # pieces a placed segment meets
    assert min(spans) >= 1 and max(spans) >= 4 and sum(x >= 3 for x in spans) > 0.9 * len(spans)
    assert max(e for l in lists for _, e in l) > T - 200


def test_long_list_top_is_long():
    lists, _ = R.oracle_of("long_list_top", R.ANNOTATOR)
    assert min(len(l) for l in lists) > 1024               # beyond k_consolidate's lists: k_merge_big and what follows it
    assert max(e for l in lists for _, e in l) > T - 400


@pytest.mark.parametrize("name", ["top_tiny_b1", "top_tiny_b3", "wide_span"])
def test_annotation_track_ends_at_T(name):
    c = R.for_sampler(R.in_domain()[name], R.ANNOTATOR)
    assert c.annos[0][-1][1] == T
    lists, _ = R.oracle_of(name, R.ANNOTATOR)
    counts = R.oracle_counts(c, R.ANNOTATOR, lists)
    for k, counter in enumerate(R.COUNTERS):
        assert counts[k].shape == (1, c.samples) and counts[k].any(), counter
    # the last annotation interval is hit: some sampled base lies in it
    lo = c.annos[0][-1][0]
    assert any(e > lo for l in lists for _, e in l)


def test_oracle_equals_the_reference_on_the_goldens():
    """every in-domain stream of tests/golden/coordinate_range.json: the oracle's list is the reference's, and the oracle's
    generator stands where the reference's stood.  The inputs recorded are the cases' as they are today."""
    doc = R.load_golden()
    cases = R.in_domain()
    n = at_T = 0
    for g in doc["in_domain"]:
        c = cases[g["case"]]
        segs, ws = [tuple(x) for x in g["segments"]], [tuple(x) for x in g["workspace"]]
        assert [(segs, ws)] == c.units and g["bucket_size"] == c.bucket_size, g["case"]
        for seed, flat, nxt in g["streams"]:
            one = c._replace(seed=seed, samples=1)
            rng = O.RandomState(seed)
            if g["sampler"] == R.ANNOTATOR:
                got = O.aslist(O.sampler_annotator(rng, segs, ws, c.bucket_size, R.NBUCKETS)[0])
            elif g["sampler"] == R.SEGMENTS:
                got = O.aslist(O.sampler_segments(rng, segs, ws, c.bucket_size, R.NBUCKETS))
            else:
                got = R.BM.sample(rng, segs, ws, bucket_size=c.bucket_size, nbuckets=R.NBUCKETS)
            assert got == list(zip(flat[0::2], flat[1::2])), (g["case"], g["sampler"], seed)
            assert rng.u32() == nxt, (g["case"], g["sampler"], seed)
            assert got == R.oracle_units(one, g["sampler"])[0][0]
            at_T += sum(e == T for e in flat[1::2]) if (g["case"], g["sampler"]) == ("top_tiny_b1", R.ANNOTATOR) else 0
            n += 1
    assert n >= 400 and at_T == 6
    assert {(g["case"], g["sampler"]) for g in doc["in_domain"]} >= {(name, k) for name in ("top_tiny_b1", "bottom", "wide_span", "frag_top")
                                                                     for k in LIST_SAMPLERS}


def test_the_reference_past_the_border_is_on_record():
    """evidence only (nothing is expected of the library here but the refusal): past the border the reference raised on
    3, 11, 8 and 30 streams: at gat/Engine.pyx:596 (intersected_segments.sum() <= unintersected_segments.sum()) on 46 of them,
    at :307 (SegmentListSampler.sample's "range error", on the list being trimmed) on the other 6."""
    runs = {g["case"]: g for g in R.load_golden()["past_border"]}
    raised = {name: len(g["raised"]) for name, g in runs.items()}
    assert raised == {"top_tiny_one_base_past": 3, "top_tiny_last_piece_at_T": 11, "top_tiny_sized_for_bucket_1_run_with_3": 8,
                      "long_segments_at_the_top": 30}
    for g in runs.values():
        assert g["highest_end_minus_T"] > 0
        assert all(r[1:3] == ["AssertionError", "Engine.pyx"] and r[3] in (596, 307) for r in g["raised"])
    lines = [r[3] for g in runs.values() for r in g["raised"]]
    assert lines.count(596) == 46 and lines.count(307) == 6 and all(r[3] == 596 for r in runs["long_segments_at_the_top"]["raised"])
