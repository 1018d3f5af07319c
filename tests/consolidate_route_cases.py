"""The first consolidation (sort + merge(0)) of sampled lists from 513 segments to beyond LDS: the problems that sit on the
borders of its routes, the plan the host must make for each, and what the oracle alone says about them.  TEST INFRASTRUCTURE
ONLY, no GPU import: tests/test_consolidate_route_cases_model.py checks the table on the oracle, tests/test_consolidate_routes_gpu.py
runs it on the device and compares lists, counts, gat_sampler_last_launch's report and the unit accounting.

The rules the borders follow, each read from the code (n: a unit's working segments, hist_total; cap: its slab region):

  cap_for            cap = roundup64(n + n / 4 + 96)                              gat_prep_units.h:170, cap_for()
  size classes       launch order = n descending; a new class where cap * 10 <= first cap of the class * 7, six at most
                                                                                  gat_prep.hip:842, upload_layout()
  split path         max n + max n / 8 <= 1024 (and not huge): k_consolidate, k_tail
                                                                                  gat_prep.hip:1184, split_path_pays()
  long lists         max n + max n / 8 > 1024 (and not huge); a unit is long by the same rule
                                                                                  gat_mi355.hip:535 and :540, plan_batch()
  huge               (640 state words + 2 * max cap) * 4 bytes > 160 KiB          gat_mi355.hip:530-531, plan_batch()
  merge_big          2 * max cap * 4 + (nbk + 1) * 4 + 1024 <= 160 KiB, nbk = the power of two from 1 024 to 8 192 that
                     reaches max cap                                              gat_mi355.hip:537-541, plan_batch()
  big_buckets        without merge_big: the largest of nbk, nbk / 2, .. >= 1 024 with k_sampler's LDS + (buckets + 1) * 4
                     <= 160 KiB, else 0                                           gat_mi355.hip:549-551, plan_batch()
  k_merge_big ccap   per class, n0 its first unit's n: min(cap, roundup64(n0 + n0 / 12 + 64))
                                                                                  gat_mi355.hip:799-800, enqueue_long_lists()
  k_merge_big form   per = ceil(ccap / 512 threads): <= 8 -> 8, <= 16 -> 16, <= 24 -> 24 elements a thread in registers,
                     else 0 (the two-pass form)                                   gat_mi355.hip:805-806, enqueue_long_lists()
  k_merge_big buckets  register forms: 1 024 doubled while 2 * b + 512 + 1 <= ccap and 2 * b <= 8 192; form 0: 8 192 halved
                     while above 1 024 and (half of it >= ccap or fewer workgroups fit a CU's 160 KiB than with 1 024)
                                                                                  gat_mi355.hip:801-811, enqueue_long_lists()
  k_merge_big's own  a list of n <= 1 024 or n > ccap is left alone, and one whose fullest bucket holds more than 48
                                                                                  gat_kernels.h:1431, :1520 and :1707
  k_consolidate ccap one launch for all classes (calls of <= 1 024 tiles): min(cap, min(max cap, 1 280),
                     roundup32(n0 + n0 / 12 + 64)); its LDS adds 528 scratch words
                                                                                  gat_mi355.hip:872-891, enqueue_split_path()
  tail_big ..        behind merge_big, no split path, workspaces of <= 64 pieces: k_tail_big, k_resume_big, k_queue_rest
                                                                                  gat_mi355.hip:544-546, plan_batch()
  TREE               some workspace of more than 32 pieces                        gat_types.h:12, kWsTreeMin
  k_sampler variant  (long lists: 2) + (TREE: 1); 6 + TREE huge; 8: variant 0 with 20 waves' LDS in 160 KiB
                                                                                  gat_mi355.hip:937-940, enqueue_sampler()

split path and long lists exclude each other (both ask max n + max n / 8), so k_consolidate never runs behind k_merge_big
without a knob: a unit of 912..1 024 segments (911 + 911 / 8 is 1 024) is k_merge_big's when its sample placed more than
1 024 and k_sampler's (queued by k_queue_rest) when not -- both in one launch, the cases a912 .. a1024.

What the device decides per (sample, unit) is not in the report; it follows from the PLACED count -- the list's length at
the first consolidation, placed_counts() below from a replay of the reference's loop on the oracle's generator --:
k_merge_big takes a list of 1 024 < placed <= ccap whose fullest bucket holds <= 48, everything else stays k_sampler's.  A
unit k_merge_big declined is never carried by k_tail_big: n_tail_units <= the (sample, unit)s within those bounds.

`direct` (fewer positions than buckets: the bucket of a start is its distance from the lowest possible start): a placement
covers at least one base of the workspace that the loop still counts as missing, so a list of n placements needs a workspace
of more than n bases, and the span the sorts bucket is the workspace's extent (+ the longest length in k_merge_big, which
takes it from the workspace).  The sorts of 513..1 024 elements (k_consolidate, k_sampler) have 512 buckets: never `direct`.
k_merge_big's register forms have up to 8 192 buckets from ccap 8 705 on (n0 from 7 977), so a unit of 7 977..8 190
one-base segments side by side (normalize does not join neighbours that only touch) in a workspace of fewer than 8 190
bases IS sorted `direct`: c_direct8192, compacting and loose; merge_span() and merge_nb() below say so for every sample.
a_direct* and c_direct are the dense shape at the other lengths (one-base segments every other base: two positions per
element, runs of equal starts), not `direct`.

Rows: k_tail_big and k_resume_big hold no generator; a unit whose pre-generated rows end behind k_merge_big's consolidation
is redone from its seed (n_full_units; tests/test_rows_run_out_gpu.py).  Only the dense c_direct* cases draw past their
rows -- half or all of their workspace is covered, every round is mostly rejected --: used_outputs() counts their
streams' raw outputs from a full replay, NEEDS_ROWS names them, everywhere else n_full_units is 0.
"""
import collections
import functools

import numpy as np

import brute_force_model as BM
from oracle import oracle as O

SEED = 77
NBUCKETS = 100000
OVERLAP = ("nucleotide-overlap", "segment-overlap")          # segment-overlap: final lists, k_resume_big<false> compacts
LOOSE = ("nucleotide-overlap", "nucleotide-density")         # with GAT_MERGED_MIN_TRACKS=1: k_count_merged, k_resume_big<true>
MAX_QUEUED = 0.15                                            # tests/test_consolidate_sort.py: the share k_tail may leave of spread lists

MAX_LDS = 160 * 1024
MT_WORDS = 640               # kMtLdsWords
SORT_WORDS = 528             # kSortScratchWords
MERGE_THREADS = 512          # kMergeThreads
WS_TREE_MIN = 32             # kWsTreeMin
TAIL_MAX_WS = 64             # kTailMaxWs
MAX_CLASSES = 6              # GAT_SIZE_CLASSES
REPORT_CLASSES = 8           # GAT_SAMPLER_REPORT_CLASSES
MAX_BUCKET = 48              # k_merge_big: a fuller bucket and the list is left to k_sampler


def _up(x, m):
    return (x + m - 1) // m * m


def cap_for(n):
    return _up(n + n // 4 + 96, 64)


def merge_ccap(n0):
    return min(cap_for(n0), _up(n0 + n0 // 12 + 64, 64))


def merge_form(ccap):
    per = (ccap + MERGE_THREADS - 1) // MERGE_THREADS
    return 8 if per <= 8 else 16 if per <= 16 else 24 if per <= 24 else 0


def merge_buckets(ccap):
    if merge_form(ccap) > 0:
        b = 1024
        while 2 * b + MERGE_THREADS + 1 <= ccap and 2 * b <= 8192:
            b *= 2
        return b

    def wgs_at(b):
        return MAX_LDS // (2 * ccap * 4 + (b + 1) * 4 + 1024)
    b = 8192
    while b > 1024 and (b // 2 >= ccap or wgs_at(b) < wgs_at(1024)):
        b //= 2
    return b


def is_long(n):
    return n + n // 8 > 1024


def plan(ns, max_nws=1, samples=64):
    """gat_sampler_report as the rules above give it for a problem of units with ns working segments (a contig each or
    not: the plan does not ask), its longest workspace of max_nws pieces, and a call of `samples` samples in one batch --
    without the call's own part (resume_virtual)."""
    order = sorted(ns, reverse=True)
    caps = [cap_for(n) for n in order]
    starts, first = [], 0
    for i, c in enumerate(caps):
        if i == 0 or (c * 10 <= first * 7 and len(starts) < MAX_CLASSES):
            starts.append(i)
            first = c
    max_cap, max_n = caps[0], order[0]
    lds = (MT_WORDS + 2 * max_cap) * 4
    R = collections.OrderedDict()
    R["huge"] = int(lds > MAX_LDS)
    if R["huge"]:
        lds = MT_WORDS * 4
    R["tree"] = int(max_nws > WS_TREE_MIN)
    R["split"] = int(max_n + max_n // 8 <= 1024 and not R["huge"])
    R["long_lists"] = int(not R["huge"] and is_long(max_n))
    R["merge_big"] = R["tail_big"] = R["resume_big"] = R["long_queue"] = R["big_buckets"] = R["n_long"] = 0
    classes = [dict(first=s, merge_ccap=0, merge_buckets=0, merge_form=-1, consolidate_ccap=0) for s in starts[:REPORT_CLASSES]]
    if R["long_lists"]:
        nbk = 1024
        while nbk < max_cap and nbk < 8192:
            nbk *= 2
        R["n_long"] = sum(1 for n in order if is_long(n))
        R["merge_big"] = int(2 * max_cap * 4 + (nbk + 1) * 4 + 1024 <= MAX_LDS)
        if R["merge_big"]:
            R["tail_big"] = R["resume_big"] = R["long_queue"] = int(max_nws <= TAIL_MAX_WS)
            for c, k in zip(classes, starts):
                if k < R["n_long"]:
                    ccap = merge_ccap(order[k])
                    c.update(merge_ccap=ccap, merge_buckets=merge_buckets(ccap), merge_form=merge_form(ccap))
        else:
            while nbk >= 1024 and lds + (nbk + 1) * 4 > MAX_LDS:
                nbk //= 2
            if nbk >= 1024:
                R["big_buckets"] = nbk
                lds += (nbk + 1) * 4
    if R["split"]:
        assert ((samples + 63) // 64) * len(ns) <= 1024          # one launch for all classes
        ccap = min(caps[0], min(max_cap, 1280), _up(order[0] + order[0] // 12 + 64, 32))
        assert (SORT_WORDS + 2 * ccap) * 4 <= MAX_LDS
        for c in classes:
            c["consolidate_ccap"] = ccap
    R["sampler_variant"] = (6 + R["tree"]) if R["huge"] else 2 * R["long_lists"] + R["tree"]
    if R["sampler_variant"] == 0 and lds * 20 <= MAX_LDS:
        R["sampler_variant"] = 8
    R["n_classes"] = len(starts)
    R["classes"] = classes
    return R


def _last(pred, lo, hi):
    """the last n in [lo, hi) with pred(n), pred being true up to a border and false behind it"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def borders():
    """the last n on the near side of every border above 1 024, from the rules (one unit per problem)"""
    B = collections.OrderedDict()
    B["ccap4096"] = _last(lambda n: merge_ccap(n) <= 4096, 2000, 6000)                # REGS 8 | 16
    B["ccap8192"] = _last(lambda n: merge_ccap(n) <= 8192, 5000, 10000)               # REGS 16 | 24
    B["ccap12288"] = _last(lambda n: merge_ccap(n) <= 12288, 9000, 13000)             # REGS 24 | 0
    B["merge_big"] = _last(lambda n: plan([n])["merge_big"] == 1, 9000, 20000)        # k_merge_big | k_sampler's own sort
    for b in (4096, 2048, 1024):
        B["big_buckets%d" % b] = _last(lambda n: plan([n])["merge_big"] == 1 or plan([n])["big_buckets"] >= b, 9000, 20000)
    B["lds"] = _last(lambda n: plan([n])["huge"] == 0, 9000, 30000)                   # list in LDS | in global memory
    return B


# ------------------------------------------------------------------------------------------------ geometry
def _spread(n, seed, coverage=0.002, lo=20, hi=200):
    """n segments of lo..hi bases on one workspace piece they cover `coverage` of (tests/test_consolidate_sort.py)"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(lo, hi + 1, size=n)
    size = int(lens.sum() / coverage)
    starts = np.sort(rs.choice(size // (hi + 1), size=n, replace=False)) * (hi + 1)
    return [(int(s), int(s + l)) for s, l in zip(starts, lens)], [(0, size)]


def _short(n, seed, lo, hi, origin=1000):
    """n segments of lo..hi bases side by side from `origin` on (tests/test_consolidate_sort.py)"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(lo, hi + 1, size=n)
    starts = origin + np.arange(n) * (hi + 1)
    return [(int(s), int(s + l)) for s, l in zip(starts, lens)]


def _cut(unit, pieces):
    """the unit with its one workspace piece cut into `pieces`: gaps of 10 bases in the widest stretches between segments"""
    segs, ((w0, w1),) = unit
    gaps = sorted(((b[0] - a[1], a[1]) for a, b in zip(segs, segs[1:])), reverse=True)[:pieces - 1]
    assert len(gaps) == pieces - 1 and gaps[-1][0] >= 30
    ws, at = [], w0
    for _, end in sorted(gaps, key=lambda g: g[1]):
        ws.append((at, end + 10))
        at = end + 20
    ws.append((at, w1))
    return segs, ws


def _moved(unit, offset):
    segs, ws = unit
    return [(s + offset, e + offset) for s, e in segs], [(s + offset, e + offset) for s, e in ws]


def _uneven(n, n_long, long_len, seed):
    """n segments, n_long of them of long_len bases and the rest of 10, spread over a workspace they cover 1 % of: the
    count of placements up to the first consolidation -- a renewal count -- spreads by cv(length) * sqrt(n)"""
    rs = np.random.RandomState(seed)
    lens = np.full(n, 10)
    lens[rs.choice(n, size=n_long, replace=False)] = long_len
    size = int(lens.sum() / 0.01)
    starts = np.sort(rs.choice(size // (long_len + 1), size=n, replace=False)) * (long_len + 1)
    return [(int(s), int(s + l)) for s, l in zip(starts, lens)], [(0, size)]


# ------------------------------------------------------------------------------------------------ the cases
# units: (segments, workspace) each, a contig of its own unless `iso` (then units 0 and 1 are the two isochore classes of
#   contig 0, and gat_sample returns contig lists made by k_contig)
# verdict: what k_merge_big does with the long units' lists -- "short" no unit is long; "take" every list within its bounds;
#   "decline" none (crowded buckets); "both" some samples on either side of `straddle`, the placed count that decides
# spread: lists that cover 0.2 % of their workspace (the gates' units 1 %) -- whatever takes them carries them on
Case = collections.namedtuple("Case", "name group units S counters loose iso verdict straddle spread pair")


def _case(name, group, units, S, counters=OVERLAP, iso=False, verdict="take", straddle=None, spread=False, pair=None):
    if isinstance(units, tuple):
        units = [units]
    return Case(name, group, units, S, tuple(counters), tuple(counters) == LOOSE, iso, verdict, straddle, spread, pair)


def _group_a():
    out = []
    for n in (520, 700, 905, 910, 911, 912, 960, 1000, 1016, 1024):
        # (the placed count of a spread list is n +- cv(length) sqrt(n) = 15: the lists of 1 016 and 1 024 segments lie on both
        #  sides of 1 024, those of up to 1 000 below it)
        out.append(_case("a%d" % n, "a", _spread(n, 2000 + n), 70, spread=True,
                         verdict=("both" if n >= 1016 else "take") if is_long(n) else "short", straddle=1024 if n >= 1016 else None))
    for n in (600, 1000):
        v = "take" if is_long(n) else "short"
        w = 10 * n                       # (the segments take 6 n bases of the first piece)
        # two crowded buckets, the rest empty
        out.append(_case("a_cap%d" % n, "a", (_short(n, 7 + n, 1, 5), [(1000, 1000 + w), (1500000000, 1500000000 + w)]), 70, verdict=v))
        # 11 buckets of 512 a piece (the pieces 46 pieces apart), 22 in all: 27 and 45 members each
        out.append(_case("a_crowded%d" % n, "a", (_short(n, 8 + n, 1, 5), [(1000, 1000 + w), (1000 + 46 * w, 1000 + 47 * w)]), 70, verdict=v))
        # one-base segments every other base in a workspace of 2 n + 100 bases: two positions per element, runs of equal starts
        out.append(_case("a_direct%d" % n, "a", (_short(n, 12 + n, 1, 1), [(1000, 1100 + 2 * n)]), 70, verdict=v))
        # a long piece beside fifty fragments a bucket apart or more
        # (99 of 512 buckets with 6 or 10 members each, under the sorts' cap of 16; the fragments eight buckets apart, a bucket wide)
        segs, ((_, size),) = _spread(n, 10 + n, lo=20, hi=100)
        out.append(_case("a_mix%d" % n, "a", (segs, [(0, size)] + [(size + size // 12 * (k + 1), size + size // 12 * (k + 1) + size // 100) for k in range(50)]),
                         70, verdict=v))
    return out


def _group_b():
    B = borders()
    out = []
    sizes = []
    for key in ("ccap4096", "ccap8192", "ccap12288"):
        sizes += [(key + "_last", B[key]), (key + "_first", B[key] + 1)]
    top0 = B["merge_big"]
    sizes.append(("regs0_mid", (B["ccap12288"] + 1 + top0) // 2))
    for tag, n in sizes:
        S = 70 if merge_ccap(n) <= 4096 else 8
        unit = _spread(n, 3000 + n)
        pair = tag.replace("_last", "").replace("_first", "") if tag != "regs0_mid" else None
        out.append(_case("b_%s" % tag, "b", unit, S, spread=True, pair=pair))
        out.append(_case("b_%s_loose" % tag, "b", unit, S, counters=LOOSE, spread=True))
    # the last register slot of a thread (elements ccap - 512 .. ccap - 1) and the top of the 14 bits a bucket's first slot is
    # packed into: a spread list places n +- 0.5 %, a twelfth short of ccap; with one segment in 25 of 1 500 bases instead of
    # 10 the placed count spreads by 4 % (cv(length) 4.2) -- some samples in the last slot, some beyond ccap (declined)
    for tag, key in (("regs16_top", "ccap8192"), ("regs24_top", "ccap12288")):
        out.append(_case("b_%s" % tag, "b", _uneven(B[key], B[key] // 25, 1500, 31), 16, verdict="both", straddle=merge_ccap(B[key])))
    # TREE: 40 workspace pieces (more than kWsTreeMin, within k_tail_big's 64) at a REGS 8 and a REGS 24 size
    for tag, n, S in (("regs8_tree", 3000, 70), ("regs24_tree", 9000, 8)):
        out.append(_case("b_%s" % tag, "b", _cut(_spread(n, 3000 + n), 40), S, spread=True))
    return out


DIRECT_N = 8000
NEEDS_ROWS = ("c_direct", "c_direct8192", "c_direct8192_loose")       # the streams of these draw past their rows (see above)
# GAT_RNG_SLACK (the factor on a stream's expected outputs, default 1) for the *_rows cases: their streams use 4 to 4.2 times
# their default rows (c_direct 8 550 of 6 512 .. c_direct8192 104 400 of 24 976, printed by the GPU test)
MORE_ROWS = {"c_direct_rows": "6", "c_direct8192_rows": "6", "c_direct8192_rows_loose": "6"}


def base_name(name):
    """the case with the same problem and streams: without _loose (other counters) and _rows (more rows)"""
    for suffix in ("_loose", "_rows"):
        if name.endswith(suffix):
            name = name[:-len(suffix)]
    return name


def _side_by_side(n, width):
    """n one-base segments on consecutive bases in the middle of one workspace piece of `width` bases"""
    assert merge_buckets(merge_ccap(n)) == 8192 and merge_form(merge_ccap(n)) == 24 and width + 2 < 8192 and n < width
    at = 1000 + (width - n) // 2
    return [(at + i, at + i + 1) for i in range(n)], [(1000, 1000 + width)]


def _group_c():
    n = 1500
    w = 10 * n
    return [
        # two short pieces 1.5e9 apart: two buckets of 1 024 hold 750 each
        _case("c_clustered", "c", (_short(n, 21, 1, 5), [(1000, 1000 + w), (1500000000, 1500000000 + w)]), 70, verdict="decline"),
        # one-base segments every other base: dense, three positions per bucket, runs of equal starts (not `direct`: see above)
        _case("c_direct", "c", (_short(n, 22, 1, 1), [(1000, 1100 + 2 * n)]), 70, verdict="take"),
        # `direct`: 8 000 one-base segments side by side in 8 100 bases -- 8 192 buckets, a position each (see above)
        _case("c_direct8192", "c", _side_by_side(DIRECT_N, 8100), 8, verdict="take"),
        _case("c_direct8192_loose", "c", _side_by_side(DIRECT_N, 8100), 8, counters=LOOSE, verdict="take"),
        # the three again with rows for every stream (MORE_ROWS): k_tail_big and k_resume_big finish the units FROM k_merge_big's
        # list -- without them the unit is redone from its seed and what k_merge_big sorted is thrown away
        _case("c_direct_rows", "c", (_short(n, 22, 1, 1), [(1000, 1100 + 2 * n)]), 70, verdict="take"),
        _case("c_direct8192_rows", "c", _side_by_side(DIRECT_N, 8100), 8, verdict="take"),
        _case("c_direct8192_rows_loose", "c", _side_by_side(DIRECT_N, 8100), 8, counters=LOOSE, verdict="take"),
        # 1 440 segments of 10 bases and 60 of 1 500: cv(length) = 4.2, the placed count spreads by 160 around 1 500 -- beyond
        # ccap = 1 728 in some samples, within it in others (and within the slab region's 1 984 in all: no overflow, no retry;
        # the model test asserts all three)
        _case("c_longer", "c", _uneven(n, 60, 1500, 23), 128, verdict="both", straddle=merge_ccap(n)),
    ]


def _gate_unit(n, seed):
    return _spread(n, seed, coverage=0.01, lo=10, hi=40)        # (mean length 25, as test_hip_parity's very_large_unit)


def _group_d():
    B = borders()
    out = []
    for key in ("merge_big", "big_buckets4096", "big_buckets2048", "big_buckets1024", "lds"):
        for side, n in (("last", B[key]), ("first", B[key] + 1)):
            out.append(_case("d_%s_%s" % (key, side), "d", _gate_unit(n, 4000 + n), 4, spread=True, pair=key))
    # a unit just above a problem-wide gate beside short and long units that did nothing to deserve its route
    for tag, n, iso in (("merge_big", B["merge_big"] + 1, True), ("lds", B["lds"] + 1, False)):
        units, at = [], 0
        for m in (300, 700, 950, 2000, 5000, n):
            u = _moved(_gate_unit(m, 5000 + m), at)
            at = u[1][-1][1] + 1000000
            units.append(u)
        out.append(_case("d_mixed_%s" % tag, "d", units, 4, iso=iso, spread=True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    cs = _group_a() + _group_b() + _group_c() + _group_d()
    out = collections.OrderedDict((c.name, c) for c in cs)
    assert len(out) == len(cs)
    return out


def names(group):
    return [c.name for c in cases().values() if c.group == group]


# ------------------------------------------------------------------------------------------------ the oracle's side
def _annos(ws):
    """one track: the first 500 bases of the workspace, a tenth of it in its middle, its last 300 bases"""
    lo, hi = ws[0][0], ws[-1][1]
    mid = (lo + hi) // 2
    return [(lo, lo + 500), (mid, mid + (hi - lo) // 10), (hi - 300, hi)]


def flat_of(case):
    units = case.units
    if len(units) == 1 and not case.iso:
        # (as _flat() of tests/test_consolidate_sort.py: the one track is the workspace itself)
        s, w = O.segs(units[0][0]), O.segs(units[0][1])
        return dict(n_units=1, segs=s, seg_off=[0, len(s)], ws=w, ws_off=[0, len(w)], unit_contig=[0], n_contigs=1,
                    merge_contigs=0, n_tracks=1, annos=w, anno_off=[0, len(w)], cws_nseg=[len(w)], bucket_size=1, nbuckets=NBUCKETS)
    n = len(units)
    contig = [0, 0] + list(range(1, n - 1)) if case.iso else list(range(n))
    cws = [[] for _ in range(contig[-1] + 1)]
    for c, (_, w) in zip(contig, units):
        cws[c] += w
    cws = [O.aslist(O.normalize(sorted(w))) for w in cws]
    annos = [_annos(w) for w in cws]
    segs = O.segs([x for s, _ in units for x in s])
    ws = O.segs([x for _, w in units for x in w])
    return dict(n_units=n, segs=segs, seg_off=np.concatenate([[0], np.cumsum([len(s) for s, _ in units])]).astype(np.int64),
                ws=ws, ws_off=np.concatenate([[0], np.cumsum([len(w) for _, w in units])]).astype(np.int64),
                unit_contig=np.array(contig, np.int32), n_contigs=len(cws), merge_contigs=int(case.iso), n_tracks=1,
                annos=O.segs([x for a in annos for x in a]),
                anno_off=np.concatenate([[0], np.cumsum([len(a) for a in annos])]).astype(np.int64),
                cws_nseg=np.array([len(w) for w in cws], np.int64), bucket_size=1, nbuckets=NBUCKETS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(flat, counts, (segments, offsets)) of the oracle for samples [0, S): computed once per case, shared, never modified"""
    case = cases()[name]
    flat = flat_of(case)
    want, wsamples = O.run_samples(flat, list(case.counters), SEED, 1, 0, case.S, want_samples=True)
    for a in list(want) + list(wsamples):
        a.setflags(write=False)
    return flat, want, wsamples


def working(case):
    """every unit's working segments (hist_total)"""
    return [len(O.filter(s, w)) for s, w in case.units]


def expected_plan(name):
    case = cases()[name]
    return plan(working(case), max(len(w) for _, w in case.units), case.S)


@functools.lru_cache(maxsize=None)
def placed_counts(name):
    """[sample][unit]: the list's length at the first consolidation -- SamplerAnnotator.sample (gat/Engine.pyx:515-606) up to
    there on the oracle's generator, stream (SEED + s * n_units + u) as rows_cases.replay_annotator has it in full"""
    if base_name(name) != name:
        return placed_counts(base_name(name))
    case = cases()[name]
    nu = len(case.units)
    prep = []
    for segs, ws in case.units:
        work = O.aslist(O.filter(segs, ws))
        hist, bucket = O.length_distribution(work, 1, NBUCKETS)
        cdf, total = [], 0
        for a, b in ws:
            total += b - a
            cdf.append(total - 1)
        prep.append((BM.HistogramSampler(hist, bucket), O.total(O.intersect(work, ws)), [tuple(x) for x in ws], cdf, total))
    out = []
    for s in range(case.S):
        row = []
        for u, (hs, ltotal, ws, cdf, total) in enumerate(prep):
            rng = O.RandomState((SEED + s * nu + u) & 0xFFFFFFFF)
            remaining, n = ltotal, 0
            while True:
                length = hs.sample(rng)
                if remaining <= length:
                    break
                remaining -= BM.sls_sample(rng, ws, cdf, total, length)[2]
                n += 1
            row.append(n)
        out.append(tuple(row))
    return tuple(out)


def merge_span(case, u=0):
    """the span k_merge_big buckets unit u's starts over: from the workspace's start less the longest length + 1 (or 0) to
    its end (gat_kernels.h:1459-1466; bucket_size 1)"""
    segs, ws = case.units[u]
    max_len = max(e - s for s, e in segs) + 1
    return ws[-1][1] - max(0, ws[0][0] - max_len)


def merge_nb(placed, buckets):
    """k_merge_big's buckets for a list of `placed`: 1 024 doubled while below the list and the launch's bound (:1468-1469)"""
    nb = 1024
    while nb < placed and nb < buckets:
        nb *= 2
    return nb


@functools.lru_cache(maxsize=None)
def used_outputs(name):
    """per sample of a one-unit case: the raw MT19937 outputs its stream consumes up to the consolidation that ends the loop
    (the device's count: rows_cases.replay_annotator, checked there against the oracle's list and draws)"""
    import rows_cases as RC
    if base_name(name) != name:
        return used_outputs(base_name(name))
    case = cases()[name]
    (segs, ws), = case.units
    _, _, (seg, off) = reference(name)
    out = []
    for s in range(case.S):
        r = RC.replay_annotator((SEED + s) & 0xFFFFFFFF, segs, ws, 1)
        assert r[0] == O.aslist(seg[off[s]:off[s + 1]]), (name, s)
        out.append(r[3])
    return tuple(out)


def fullest_bucket(case, u, nb=1024):
    """the most starts any of k_merge_big's nb position buckets over unit u's workspace can expect: the share of the
    workspace's bases in one bucket times the unit's segments"""
    segs, ws = case.units[u]
    lo, hi = ws[0][0], ws[-1][1]
    width = max(1, (hi - lo) // nb)
    per = collections.Counter()
    for a, b in ws:
        for k in range((a - lo) // width, (b - 1 - lo) // width + 1):
            per[k] += min(b, lo + (k + 1) * width) - max(a, lo + k * width)
    return max(per.values()) / float(sum(b - a for a, b in ws)) * len(segs)


def takeable(name):
    """per unit in problem order: the samples whose list k_merge_big can take -- the unit is long, 1 024 < placed <= the ccap
    of its size class, and the case's keys are not crowded.  None where the plan launches no k_merge_big."""
    case = cases()[name]
    ns = working(case)
    P = plan(ns, max(len(w) for _, w in case.units), case.S)
    if not P["merge_big"]:
        return None
    order = sorted(range(len(ns)), key=lambda u: (-ns[u], u))
    ccap = {}
    for pos, u in enumerate(order):
        cls = max(k for k, c in enumerate(P["classes"]) if c["first"] <= pos)
        ccap[u] = P["classes"][cls]["merge_ccap"] if pos < P["n_long"] else 0
    placed = placed_counts(name)
    return [sum(1 for row in placed if 1024 < row[u] <= ccap[u]) if case.verdict != "decline" else 0 for u in range(len(ns))]
