"""The cases and sweep tables of tests/rows_cases.py on the oracle alone (no device): every stream needs more outputs than
the largest row count its sweep asks for, the mixed row count splits the streams, the lists fall into the sort class the
case is named for, and the tables hold the switch positions they claim.  A case or table that stops doing what the GPU
tests (tests/test_rows_run_out_gpu.py) need it for fails here."""
import pytest

import rows_cases as RC
from oracle import oracle as O

SINGLE = ["small", "small_b3", "mid", "mid_simple", "mid_grid", "large", "long"]


def test_cases_are_what_the_budget_rule_needs():
    """one unit per problem (rows_per_sample() is the unit's row count), normalized, every segment working; `small` within
    the 65 working segments below which the spread term is 0; mid_simple one piece with no power of two between its
    position and offset ranges (k_place_scan's cm_ok); mid_grid beyond kPlaceWsLds = 256 pieces; small_b3 bucket 3"""
    cases = RC.cases()
    for name in SINGLE:
        c = cases[name]
        assert len(c.units) == 1 and not c.isochores, name
    for name, c in cases.items():
        for segs, ws in c.units:
            assert O.check(segs) and O.check(ws) and len(O.filter(segs, ws)) == len(segs), name
    assert len(cases["small"].units[0][0]) <= 64 and cases["small_b3"].bucket_size == 3
    (s_segs, s_ws), = cases["mid_simple"].units
    width, lmax = s_ws[0][1] - s_ws[0][0], max(e - s for s, e in s_segs)
    assert len(s_ws) == 1 and (width - 2 + lmax).bit_length() == (width - 1).bit_length()
    assert len(cases["mid_grid"].units[0][1]) > 256
    assert len(cases["multi"].units) == 4 and cases["multi"].isochores
    assert RC.SAMPLES == 70 and RC.BEGIN > 0                # two tiles, the second one partial; a non-zero sample_begin


@pytest.mark.parametrize("name", SINGLE)
def test_every_stream_needs_more_than_the_sweeps_ask_for(name):
    """min over the streams of the outputs the device consumes (`used`: the oracle's D less the reference's last, discarded
    placement) exceeds MAX_ROWS, and every table entry and short budget of the case is at most MAX_ROWS and at least 16"""
    st = RC.streams_of(name)
    assert len(st) == RC.SAMPLES
    assert all(0 < s.D - s.used <= 64 and s.used > RC.MAX_ROWS[name] for s in st), (name, RC.min_used(name))
    asked = {"small": RC.SMALL_ROWS, "small_b3": RC.SMALL_ROWS, "large": RC.BLOCK_ROWS,
             "mid": RC.RESIDUE_ROWS + RC.ROUTE_ROWS_DEEP + RC.ROUTE_ROWS_LATE["mid"],
             "mid_simple": RC.ROUTE_ROWS_DEEP + RC.ROUTE_ROWS_LATE["mid_simple"]}.get(name, []) + [RC.SHORT_ROWS[name]]
    assert all(16 <= r <= RC.MAX_ROWS[name] and r % 16 == 0 for r in asked), (name, asked)
    assert max(asked) == RC.MAX_ROWS[name] or name in ("mid_grid", "long")
    if name in RC.MAX_ROWS_SEGMENTS:                        # SamplerSegments: len(segments) placements, no consolidation
        sg = RC.streams_of(name, RC.SEGMENTS)
        assert all(s.used == s.D > RC.MAX_ROWS_SEGMENTS[name] for s in sg), name
        assert RC.SHORT_ROWS[name] <= RC.MAX_ROWS_SEGMENTS[name]


def test_the_mixed_row_count_splits_the_streams():
    """strictly between a quarter and three quarters of mid's streams need more than MIXED_ROWS, in both tiles; long's late
    budget ends behind the first consolidation of some streams, within the placements of others, and suffices for the rest"""
    st = RC.streams_of("mid")
    more = RC.need_more("mid", RC.MIXED_ROWS)
    assert RC.SAMPLES / 4 < more < 3 * RC.SAMPLES / 4, more
    for tile in (st[:64], st[64:]):
        assert 0 < sum(s.used > RC.MIXED_ROWS for s in tile) < len(tile)
    lg, r = RC.streams_of("long"), RC.LONG_LATE_ROWS
    done = sum(s.used <= r for s in lg)
    placing = sum(s.first_at >= r for s in lg)
    behind = sum(s.first_at < r < s.used for s in lg)
    assert min(done, placing, behind) >= 10 and done + placing + behind == RC.SAMPLES, (done, placing, behind)


def test_the_route_rows_lie_where_they_claim():
    """deep: every stream is still placing in front of its first consolidation, with at most a third of its list placed --
    the hand-over is -3; one row count is a multiple of 64 and one is not.  late: just under the shortest stream; mid_simple:
    every stream is past its first consolidation at all three; mid: nearly all at the last, some at the second, none at the
    first (-3 with nearly the whole list placed)"""
    assert sum(r % 64 == 0 for r in RC.ROUTE_ROWS_DEEP) >= 1 and sum(r % 64 != 0 for r in RC.ROUTE_ROWS_DEEP) >= 1
    for name in ("mid", "mid_simple", "mid_grid"):
        st = RC.streams_of(name)
        for r in RC.ROUTE_ROWS_DEEP + [RC.SHORT_ROWS[name]]:
            assert all(3 * r < s.first_at for s in st), (name, r)
        assert RC.min_used(name) / 5 < min(RC.ROUTE_ROWS_DEEP) and max(RC.ROUTE_ROWS_DEEP) < RC.min_used(name) / 3
    for name, want in (("mid", [(0, 0), (1, 35), (60, 70)]), ("mid_simple", [(70, 70)] * 3)):
        st = RC.streams_of(name)
        rows = RC.ROUTE_ROWS_LATE[name]
        assert len(rows) == 3 and RC.min_used(name) - 48 <= rows[0] and rows[2] < RC.min_used(name)
        for r, (lo, hi) in zip(rows, want):
            past = sum(s.first_at < r for s in st)          # the length draw in front of the first consolidation came from the rows
            assert lo <= past <= hi, (name, r, past)


@pytest.mark.parametrize("name,lo,hi", [("small", 1, 64), ("small_b3", 1, 64), ("mid", 65, 512), ("mid_simple", 65, 512),
                                        ("mid_grid", 65, 512), ("large", 513, 1024), ("long", 1025, 4000)])
def test_list_lengths_fall_into_the_sort_class(name, lo, hi):
    """the list (unintersected + sampled) at every consolidation and the oracle's final list: at most 64 (the insertion
    sort), 65..512, 513..1024, beyond 1024 (k_merge_big)"""
    for s in RC.streams_of(name):
        assert lo <= s.first_n <= hi and all(lo <= n <= hi for n in s.cons_n) and lo <= len(s.lst) <= hi, (name, s.cons_n)
        assert len(s.cons_n) >= 2                           # (a consolidation behind the first: after a switch, at the latest)


def test_multi_holds_every_class():
    """multi's four units: 65..512, at most 64, 65..512 with 300 segments, and a dozen; units 0 and 1 share a contig"""
    st = RC.streams_of("multi")
    assert len(st) == 4 * RC.SAMPLES
    for u, (lo, hi) in enumerate([(65, 512), (1, 64), (257, 512), (1, 20)]):
        assert all(lo <= n <= hi for s in st[u::4] for n in s.cons_n), u
    flat = RC.flat_of(RC.cases()["multi"], RC.ANNOTATOR)
    assert list(flat["unit_contig"]) == [0, 0, 1, 2] and int(flat["merge_contigs"]) == 1 and int(flat["n_contigs"]) == 3
    assert len(RC.contig_lists(RC.cases()["multi"], RC.lists_of("multi"))) == 3 * RC.SAMPLES


def test_the_tables_cover_what_they_claim():
    assert sorted(r % RC.MT_N for r in RC.RESIDUE_ROWS) == list(range(0, RC.MT_N, 16)) and len(RC.RESIDUE_ROWS) == 39
    assert sum(RC.RESIDUE_GROUPS, []) == RC.RESIDUE_ROWS and all(len(g) <= 8 for g in RC.RESIDUE_GROUPS)
    # rng_switch re-tempers the current block of 64 when rows % 64 != 0: both kinds, also among the residues of the last,
    # partial block (576..608), and pos = 0
    assert {r % 64 == 0 for r in RC.RESIDUE_ROWS} == {True, False}
    assert {576, 592, 608, 0} <= {r % RC.MT_N for r in RC.RESIDUE_ROWS}
    assert sorted((r // RC.MT_N, r % RC.MT_N) for r in RC.BLOCK_ROWS) == [(b, r) for b in (1, 2, 3) for r in (0, 16, 608)]
    assert sum(RC.BLOCK_GROUPS, []) == RC.BLOCK_ROWS
    assert RC.SMALL_ROWS == [16, 32, 48, 64, 80, 128, 144]
    # the second tile's rows lie at (sidx >> 6) * rows * 64: a call of more than 64 samples, and row counts that differ
    assert RC.SAMPLES > 64 and len(set(RC.RESIDUE_ROWS)) == 39


def test_large_switches_in_front_of_a_sort_of_513_to_1024():
    """at every BLOCK_ROWS entry every stream of `large` is still in front of its first consolidation, whose list has
    513..1024 segments: the first sort after the switch is of that class"""
    for s in RC.streams_of("large"):
        assert max(RC.BLOCK_ROWS) < s.first_at and 513 <= s.first_n <= 1024
