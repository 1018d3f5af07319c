"""Edge-case units for the shift (k_shift) and global permutation (k_permute) samplers, and the helpers their tests share.
TEST INFRASTRUCTURE ONLY.

A case is a list of units (segments, workspace) -- one contig per unit, no isochores, no annotations -- plus the
sampler's parameters.  The generators draw each unit from a menu of shapes chosen to reach the kernels' less travelled
branches (k_shift: windows taken whole, lists normalized in the slab, window ends on piece ends, long draw streams;
k_permute: the LDS / slab boundary at 2 048 working segments, 64-segment chunk carries, _randbelow at its bounds, W cut into
1-2 base pieces, the wrap).  The fixed units below reach each branch by construction; tests/test_sampler_edges.py checks
on the models that the generators reach what they claim, and tests/test_sampler_edges_gpu.py runs them on the device.

The models are tests/shift_model.py and tests/permutation_model.py, pinned to the reference by their known answers.
"""
import random

import numpy as np

import permutation_model as PM
import shift_model as SM
from oracle import oracle as O

SHIFT, PERM = 2, 3                      # GAT_SAMPLER_SHIFT, GAT_SAMPLER_GLOBAL_PERMUTATION
LDS_LIST = 2048                         # the LDS bound of both kernels' lists (gat_mi355.hip: the shift and permute launches)
MT_N = 624                              # words per MT19937 twist
ALL_COUNTERS = ["nucleotide-overlap", "nucleotide-density", "segment-overlap", "segment-midoverlap",
                "annotation-overlap", "annotation-midoverlap"]
# (radius, extension) pairs of the shift fuzz: radius windows narrower and wider than their segment, extension 1 (area
# 0: every window empty), odd extensions, windows of thousands of bases
SHIFT_PARAMS = [(2.0, 0), (0.5, 0), (1.0, 0), (3.7, 0), (0.1, 0), (2.0, 1), (2.0, 3), (2.0, 7), (2.0, 65), (2.0, 129),
                (2.0, 501), (2.0, 4097)]


# ------------------------------------------------------------------------------------------------ shared helpers
def rand_norm(r, n, span, maxlen, start=0):
    """up to n separated, sorted pieces in [start, span) of length at most maxlen."""
    pts = sorted(r.sample(range(start, span), 2 * n))
    out = []
    for i in range(n):
        s, e = pts[2 * i], min(pts[2 * i + 1], pts[2 * i] + maxlen)
        if e > s:
            out.append((s, e))
    return out


def units_flat(units, sampler, radius=0.0, extension=0):
    """one contig per unit, no isochores, no annotations: the sampler alone.  A unit without segments or workspace is
    skipped (gat/__init__.py:536-538): it carries contig -1 and has no contig."""
    segs = [np.array(s, dtype=np.int64).reshape(-1, 2) for s, _ in units]
    ws = [np.array(w, dtype=np.int64).reshape(-1, 2) for _, w in units]

    def cat(lst):
        a = np.concatenate(lst) if lst else np.zeros((0, 2), np.int64)
        out = np.empty(len(a), dtype=O.SEG)
        out["start"], out["end"] = a[:, 0], a[:, 1]
        return out

    def off(lst):
        return np.concatenate([[0], np.cumsum([len(x) for x in lst])]).astype(np.int64)

    n = len(units)
    live = [len(s) > 0 and len(w) > 0 for s, w in zip(segs, ws)]
    contig = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    flat = dict(n_units=n, segs=cat(segs), seg_off=off(segs), ws=cat(ws), ws_off=off(ws),
                unit_contig=contig, n_contigs=int(sum(live)), merge_contigs=0, n_tracks=0,
                annos=np.zeros(0, dtype=O.SEG), anno_off=np.zeros(1, np.int64),
                cws_nseg=np.array([len(w) for w, k in zip(ws, live) if k], np.int64), sampler=sampler)
    if sampler == SHIFT:
        flat["shift_radius"], flat["shift_extension"] = radius, extension
    return flat


class CountingRandom(random.Random):
    """random.Random that counts the 32-bit words it consumes (every draw of these samplers is getrandbits(k), k <= 32)."""

    def __init__(self, seed):
        self.words = 0
        super().__init__(seed)

    def getrandbits(self, k):
        self.words += (k + 31) // 32
        return super().getrandbits(k)


def model_units(flat, seed, s0, s1, info=None):
    """the model's (sample, unit) lists in gat_sample_units' order and the call's statistics (n_draws: 32-bit words
    consumed; n_empty_windows: shift segments with an empty window).  Unit u of sample s draws from the stream seeded
    with (seed + s * n_units + u) mod 2^32.  info, when a list, receives one dict per (sample, unit): the unit's words
    and what the model noted (shift_model.sample / permutation_model.sample stats)."""
    n, kind = int(flat["n_units"]), int(flat["sampler"])
    segs, ws = O.aslist(flat["segs"]), O.aslist(flat["ws"])
    so, wo = flat["seg_off"], flat["ws_off"]
    lists, st = [], dict(n_draws=0, n_empty_windows=0)
    for s in range(s0, s1):
        for u in range(n):
            us, uw = segs[so[u]:so[u + 1]], ws[wo[u]:wo[u + 1]]
            ust = {}
            if not us or not uw:
                lists.append([])
            elif kind == SHIFT:
                rng = O.RandomState((seed + s * n + u) & 0xFFFFFFFF)
                lists.append(SM.sample(rng, us, uw, flat["shift_radius"], flat["shift_extension"], ust))
                ust["words"] = rng.ndraws
            else:
                rng = CountingRandom((seed + s * n + u) & 0xFFFFFFFF)
                lists.append(PM.sample(rng, us, uw, ust))
                ust["words"] = rng.words
            st["n_draws"] += ust.get("words", 0)
            st["n_empty_windows"] += ust.get("empty_windows", 0)
            if info is not None:
                info.append(ust)
    return lists, st


def as_lists(seg, off):
    return [[(int(a), int(b)) for a, b in zip(seg["start"][off[i]:off[i + 1]], seg["end"][off[i]:off[i + 1]])]
            for i in range(len(off) - 1)]


def device_units(ctx, flat, seed, s0, s1):
    """the library's (sample, unit) lists of samples [s0, s1) and the call's statistics."""
    from gat_amd import _lib
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(seed, s0, s1, unit_level=True)
        return as_lists(seg, off), P.last_stats
    finally:
        P.close()


def model_counts(flat, unit_lists, counters, S):
    """the counters over the contig lists (fromIsochores: the units of a contig concatenated and merge(0)d when keys
    carry isochores), summed over contigs; float64 for nucleotide-density, int64 for the others."""
    n, nc, nt = int(flat["n_units"]), int(flat["n_contigs"]), int(flat["n_tracks"])
    annos, ao = O.aslist(flat["annos"]), flat["anno_off"]
    out = [np.zeros((nt, S), np.float64 if name == "nucleotide-density" else np.int64) for name in counters]
    for s in range(S):
        contig = [[] for _ in range(nc)]
        for u in range(n):
            c = int(flat["unit_contig"][u])
            if c >= 0:
                contig[c] += unit_lists[s * n + u]
        if int(flat["merge_contigs"]):
            contig = [O.aslist(O.merge(sorted(x), 0)) if x else [] for x in contig]
        for k, name in enumerate(counters):
            for t in range(nt):
                v = [O.counter(name, contig[c], annos[ao[t * nc + c]:ao[t * nc + c + 1]], int(flat["cws_nseg"][c]))
                     for c in range(nc) if contig[c]]
                out[k][t, s] = sum(v) if name == "nucleotide-density" else sum(int(x) for x in v)
    return out


def shift_lds_cap(flat):
    """an upper bound of k_shift's lds_cap for the launch (min(max_unit_cap, 2048, max_work + max_work/4 + 64) without the
    slab term): a unit whose raw list is longer is sorted and merged in the slab."""
    segs, ws = O.aslist(flat["segs"]), O.aslist(flat["ws"])
    so, wo = flat["seg_off"], flat["ws_off"]
    mw = 0
    for u in range(int(flat["n_units"])):
        us, uw = segs[so[u]:so[u + 1]], ws[wo[u]:wo[u + 1]]
        if us and uw:
            mw = max(mw, len(O.filter(us, uw)))
    return min(LDS_LIST, mw + mw // 4 + 64)


# ------------------------------------------------------------------------------------------------ shift
def _frag_ws(r, n, start, gaps=(0, 1, 1, 2)):
    """n pieces of 1-2 bases from `start`, separated by gaps drawn from `gaps` (0: adjacent pieces, kept apart)."""
    out, x = [], start
    for _ in range(n):
        ln = r.choice((1, 1, 2))
        out.append((x, x + ln))
        x += ln + r.choice(gaps)
    return out


def _norm(segs):
    return [tuple(x) for x in O.aslist(O.normalize(sorted(segs)))] if segs else []


def _shift_unit(r):
    kind = r.choice(("frag", "frag", "edges", "edges", "stream", "near_zero", "wide", "idle"))
    if kind == "frag":              # a fragmented workspace: windows of dozens to thousands of 1-2 base pieces
        n_ws = r.choice((70, 130, 700, 2100, 3000))
        x0 = r.choice((0, 5, 1000))
        ws = _frag_ws(r, n_ws, x0)
        hi = ws[-1][1]
        segs = []
        for _ in range(r.randint(1, 4)):
            ln = r.choice((1, 2, 3, 60, 300, 2 * hi, 3 * hi))
            s = r.randint(max(0, x0 - 50), hi + 50)
            segs.append((s, s + ln))
        return _norm(segs), ws
    if kind == "edges":             # short pieces, adjacent or 1 base apart; segments starting and ending on piece ends
        ws = []
        x = r.choice((0, 1, 3, 100))
        for _ in range(r.randint(1, 40)):
            ln = r.choice((1, 2, 5, 10, 10, 17))
            ws.append((x, x + ln))
            x += ln + r.choice((0, 0, 1, 3, 10))
        ends = sorted({p for w in ws for p in w})
        segs = []
        for _ in range(r.randint(1, 30)):
            s = r.choice(ends) + r.choice((0, 0, -1, 1))
            ln = r.choice((1, 1, 2, 3, 4, 5, 10, 20, 64, 65))
            segs.append((max(0, s), max(0, s) + ln))
        return _norm(segs), ws
    if kind == "stream":            # hundreds to a thousand working segments: two draws each, several MT twists
        span = r.choice((20000, 200000))
        ws = rand_norm(r, r.randint(1, 30), span, span)
        segs = rand_norm(r, r.randint(500, 1200), span, r.choice((1, 3, 40)))
        return segs, ws
    if kind == "near_zero":         # windows clamped at 0, starts before 0 (uint32 wrap) for backward draws
        ws = [(0, r.randint(1, 40))] + rand_norm(r, r.randint(0, 10), 400, 30, start=60)
        segs = _norm([(s, s + r.choice((1, 5, 30, 200))) for s in (r.randint(0, 30) for _ in range(r.randint(1, 6)))])
        return segs, ws
    if kind == "wide":              # a segment far longer than a small workspace: its windows taken whole
        ws = rand_norm(r, r.randint(1, 8), 3000, r.choice((1, 20, 400)))
        segs = [(r.randint(0, 100), r.randint(3000, 20000))]
        return segs, ws
    # no working segment (outside the workspace), or no segment at all
    return ([(5000, 5010)] if r.random() < 0.5 else []), [(0, 100)]


def shift_edge_units(seed):
    """(units, radius, extension) of shift case `seed`: one (radius, extension) pair and 4-7 units from the menu."""
    r = random.Random(0x5A1F7 + seed)
    radius, extension = SHIFT_PARAMS[seed % len(SHIFT_PARAMS)]
    return [_shift_unit(r) for _ in range(r.randint(4, 7))], radius, extension


def shift_fixed_units():
    """hand-built (name, units, radius, extension), one per branch of k_shift."""
    frag = [(1000 + 2 * i - i // 5, 1001 + 2 * i - i // 5) for i in range(3000)]   # 3 000 pieces of 1 base, 1 base apart
    #                                                                      # or (every fifth) adjacent: kept apart
    adj = [(10 * i, 10 * i + 10) for i in range(40)]                     # adjacent pieces (0,10),(10,20),...
    r = random.Random(17)
    many = rand_norm(r, 1700, 2_000_000, 50)
    return [
        # one segment 20 000 long, its window all 3 000 pieces: taken whole twice over (fill_all, 47 lane rounds), a raw list
        # of > 3 000 pieces while max_work is 1 (lds_cap 65): sorted and merged in the slab, adjacent pieces kept apart
        ("slab_normalize", [([(0, 20000)], frag)], 2.0, 0),
        # the same unit beside one of 1 700 working segments: lds_cap is 2 048 and the 3 000-piece list still exceeds it
        ("slab_normalize_mixed", [([(0, 20000)], frag), (many, [(0, 2_000_100)])], 2.0, 0),
        # windows of 100-odd pieces a segment 400 long overfills (extension 300: sum 150 < 400)
        ("fill_all_lanes", [([(1000 + 100 * i, 1400 + 100 * i) for i in range(0, 50, 7)], frag)], 2.0, 300),
        # window ends on piece ends (mid +- 10 on multiples of 10): zero-length ends dropped; adjacent pieces kept apart
        ("window_on_piece_ends", [([(10 * i + 5, 10 * i + 15) for i in range(0, 39, 2)], adj)], 2.0, 20),
        # extension 1: area 0, every window empty (one draw each, nothing placed)
        ("extension_one", [([(5, 9), (50, 70)], adj)], 2.0, 1),
        # radius 0.5 on 1-3 base segments: floor(length * radius / 2) = 0, empty windows
        ("zero_area", [([(3, 4), (21, 23), (44, 47)], adj)], 0.5, 0),
        # segments at 0 whose windows clamp at 0, backward draws starting before 0
        ("near_zero", [([(0, 3), (4, 40)], [(0, 2), (2, 7), (9, 60)])], 3.7, 0),
        # 900 working segments: 1 800 draws and more, three MT twists
        ("long_stream", [(rand_norm(r, 900, 100000, 20), [(0, 100000)])], 2.0, 0),
    ]


# ------------------------------------------------------------------------------------------------ permutation
PERM_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 2047, 2048, 2049)


def _free_of(r):
    """free lengths at _randbelow's edges: 0 (every draw _randbelow(1)), 2^k - 1 (free + 1 = 2^k), 2^k - 2, 2^k, large."""
    k = r.randint(1, 20)
    return r.choice((0, 0, (1 << k) - 1, (1 << k) - 1, (1 << k) - 2, 1 << k, r.randint(1, 5000),
                     (1 << 24) + r.randint(0, 1 << 20)))


def perm_unit(r, n, free, frag=None, overhang=None):
    """a unit of n segments (n working unless some are left outside the workspace) whose W has exactly `free` bases
    beyond the working segments.  frag: the free bases as 1-2 base pieces (W cut fine: segments split into many pieces);
    overhang: the workspace covers only part of some segments (W extends it by them)."""
    if frag is None:
        frag = free <= 6000 and r.random() < 0.5
    if overhang is None:
        overhang = r.random() < 0.5
    # the free bases in pieces
    if frag:
        extras, left = [], free
        while left > 0:
            ln = min(left, r.choice((1, 2)))
            extras.append(ln)
            left -= ln
    else:
        cut = sorted(r.sample(range(1, free), min(free - 1, r.randint(0, 6)))) if free > 1 else []
        extras = [b - a for a, b in zip([0] + cut, cut + [free]) if b > a]
    items = [("s", r.choice((1, 1, 2, 3, 7, 50))) for _ in range(n)] + [("f", ln) for ln in extras]
    if r.random() < 0.3:
        items += [("x", r.choice((1, 5)))]                  # a segment outside the workspace: not working
    r.shuffle(items)
    segs, ws, x = [], [], r.choice((0, 1, 1000))
    for kind, ln in items:
        x += r.choice((0, 0, 1, 2, 5))                      # 0: adjacent to the piece before (W's merge(0) unites them)
        if kind == "s":
            segs.append((x, x + ln))
            if overhang and ln > 1 and r.random() < 0.5:     # the workspace covers part of the segment only
                a = r.randint(x, x + ln - 1)
                ws.append((a, r.randint(a + 1, x + ln)))
            else:
                ws.append((x, x + ln))
        elif kind == "f":
            ws.append((x, x + ln))
        else:
            segs.append((x, x + ln))
        x += ln
    return segs, _norm_ws(ws)


def _norm_ws(ws):
    """sorted, overlaps united, adjacent pieces kept apart (SegmentList.normalize)."""
    return [tuple(x) for x in O.aslist(O.normalize(sorted(ws)))]


def perm_edge_units(seed):
    """the units of permutation case `seed`: 3-6 units of sizes and free lengths from the menus, at most one beyond
    200 working segments."""
    r = random.Random(0x9E3 + seed)
    units, big = [], False
    for _ in range(r.randint(3, 6)):
        n = r.choice(PERM_SIZES)
        if n > 200:
            if big:
                n = r.choice(PERM_SIZES[:9])
            big = True
        units.append(perm_unit(r, n, _free_of(r)))
    return units


def perm_fixed_units():
    """hand-built (name, units), one per branch of k_permute."""
    r = random.Random(23)
    small = [perm_unit(r, n, f) for n, f in ((1, 0), (5, 31), (30, 1 << 10))]
    return [
        # exactly at and one past the LDS bound, each alone in its launch (lds_cap 2 048, then 2 049 > 2 048: the slab)
        ("lds_2048", [perm_unit(r, 2048, 5000, frag=True)]),
        ("slab_2049", [perm_unit(r, 2049, 4095, frag=False)]),
        # both in one launch with small units that share its lds_cap (2 048): the 2 049 one alone keeps its arrays in the slab
        ("lds_slab_mixed", small[:2] + [perm_unit(r, 2048, 1 << 12), perm_unit(r, 2049, 300, frag=True)] + small[2:]),
        # chunk carries across 64-segment waves
        ("wave_widths", [perm_unit(r, n, f) for n, f in ((1, 14), (63, 0), (64, 63), (65, 64), (128, 127), (129, 1000))]),
        # free = 0 (_randbelow(1): every point and the shift 0, half the words rejected) and large frees
        ("free_edges", [perm_unit(r, n, f, frag=False) for n, f in ((40, 0), (300, 0), (20, (1 << 24) + 5),
                                                                    (20, (1 << 30) - 1), (700, (1 << 16) - 1))]),
        # W cut into 1-2 base pieces: every segment split many times; the wrap crossed inside segments
        ("fine_w", [perm_unit(r, 30, 3000, frag=True, overhang=True), perm_unit(r, 200, 900, frag=True)]),
    ]
