"""Inputs for the overlap-count stage, each built to reach ONE branch of its kernels, and a reference that shares no code
with them (test infrastructure only: test_count_cases_model.py proves the premises on the CPU, test_count_routes_gpu.py runs
the cases through gat_count_lists and asserts from gat_count_last_launch that the intended kernel ran).

A case is n_lists x n_groups segment lists (list l of group g at index l * n_groups + g) against n_tracks x n_groups
annotation lists (track t of group g at index t * n_groups + g), the options it sets, and what the launch report must say:
  staged / tt   k_count_seg: the tile's lists in LDS (max_m + 4 <= GAT_COUNT_LDS_ENTRIES) and the tracks of a tile
  merged        None: the nucleotide pair alone stays with k_count_seg; "any": k_count_merged in the form the build picks;
                8 / 2 / 1: k_count_merged in the form GAT_MERGED_BLOCK sets
  anno          the annotation-side kernel of the LAST list, ANNO_IDX or ANNO_PLAIN
`premise` proves on the CPU that the input has the property the case is named for.

Expected values come from oracle.counter.  The per-base model (numpy masks, written from the counters' definitions) must
agree with it wherever it applies: coordinates below MODEL_MAX, and for the two midpoint counters only where no midpoint lies in
an interval other than the first one its segment touches -- the reference's merge-join tests a segment against the FIRST
interval that ends behind its start and moves on (gat/SegmentList.pyx:1078-1146), so there the definition "the midpoint base is
in the track" and the reference differ and the oracle alone decides.
"""
import numpy as np

SEG = np.dtype([("start", "<u4"), ("end", "<u4")])
COUNTERS = ["nucleotide-overlap", "nucleotide-density", "segment-overlap", "segment-midoverlap", "annotation-overlap",
            "annotation-midoverlap"]
NUCLEOTIDE = COUNTERS[:2]
FAR = (1 << 20) - 1             # about 10^6: every shift of a grid leaves FAR in the same cell as the bases just below it
MODEL_MAX = FAR + 1024          # the per-base model is used up to here
KERNEL_SEG, KERNEL_SWAP, KERNEL_MERGED = 1, 2, 3
ANNO_NONE, ANNO_IDX, ANNO_PLAIN = 0, 1, 2
LDS_ENTRIES = 1024            # GAT_COUNT_LDS_ENTRIES' default
TRACKS_PER_BLOCK = 16         # GAT_COUNT_TRACKS_PER_BLOCK's default
LIST_SAMPLES_PER_BLOCK = 8    # a gat_count_lists launch is one sample: the smallest chunk k_count_seg is launched with
ERR_ASSERT, ERR_ARG = -2, -6


def seg(pairs):
    a = np.zeros(len(pairs), dtype=SEG)
    for i, (s, e) in enumerate(pairs):
        a[i] = (s, e)
    return a


EMPTY = seg([])


def check_list(a):
    """the library's check_list restated: None, or the error code of the first offence"""
    prev_end = None
    for s, e in zip(a["start"].tolist(), a["end"].tolist()):
        if s >= e:
            return ERR_ASSERT
        if e >= 1 << 31:
            return ERR_ARG
        if prev_end is not None and prev_end > s:
            return ERR_ASSERT
        prev_end = e
    return None


def pow2ceil(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def grid_shift(max_start, longest, grid_factor=2):
    """the position grid of a group (the rule of the annotation tables): the smallest shift with at most
    grid_factor * pow2ceil(max(16, longest list of the group)) cells up to max_start; returns (shift, cells)"""
    target = grid_factor * pow2ceil(max(16, longest))
    sh = 0
    while (max_start >> sh) + 1 > target:
        sh += 1
    return sh, (max_start >> sh) + 1


def min_cell_width(max_start, longest, grid_factor=2):
    """the bound the rule implies: a cell is at least this many bases wide"""
    return (max_start + 1) // (grid_factor * pow2ceil(max(16, longest)))


def tile_tracks(n_tracks, max_m, staged, lds_entries=LDS_ENTRIES, tracks_per_block=TRACKS_PER_BLOCK):
    """the tracks of a k_count_seg tile: at most tracks_per_block, and staged at most what fits LDS at max_m + 4 entries a list"""
    tt = min(n_tracks, tracks_per_block)
    if staged:
        tt = min(tt, lds_entries // (max_m + 4))
    return max(1, tt)


def midpoint(s, e):
    return s + (e - s) // 2


class Case(object):
    def __init__(self, name, branch, lists, annos, n_lists, n_tracks, n_groups, ws_nseg=None, options=None,
                 staged=1, tt=None, merged=None, anno=ANNO_IDX, premise=None):
        self.name, self.branch = name, branch
        self.lists, self.annos = list(lists), list(annos)
        self.n_lists, self.n_tracks, self.n_groups = n_lists, n_tracks, n_groups
        assert len(self.lists) == n_lists * n_groups and len(self.annos) == n_tracks * n_groups, name
        self.ws_nseg = list(ws_nseg) if ws_nseg is not None else [g + 1 for g in range(n_groups)]
        assert len(self.ws_nseg) == n_groups
        self.options = dict(options or {})
        self.staged, self.merged, self.anno = staged, merged, anno
        self.tt = tt if tt is not None else tile_tracks(n_tracks, self.max_m(), staged)
        self.premise = premise
        self._expected = {}

    def __repr__(self):
        return self.name

    def max_m(self):
        return max([len(a) for a in self.annos] or [0])

    def longest_list(self, l):     # noqa: E741
        return max([len(self.lists[l * self.n_groups + g]) for g in range(self.n_groups)] or [0])

    def max_coord(self):
        return max([int(a["end"][-1]) for a in self.lists + self.annos if len(a)] or [0])

    def flat(self):
        off = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)  # noqa: E731
        cat = lambda ls: np.concatenate(ls) if ls else EMPTY  # noqa: E731
        return cat(self.lists), off(self.lists), cat(self.annos), off(self.annos)

    def report(self, counters):
        """what gat_count_last_launch must say after a gat_count_lists of this case with these counters"""
        all_six = any(c not in NUCLEOTIDE for c in counters)
        if self.n_lists == 0 or self.n_tracks == 0:
            return dict(kernel=0, staged=0, hits=0, patch=0, tracks_per_block=0, samples_per_block=0, merged_form=0, anno_kernel=0)
        if not all_six and self.merged is not None:
            return dict(kernel=KERNEL_MERGED, staged=0, hits=0, patch=0, tracks_per_block=0, samples_per_block=1,
                        merged_form=self.merged, anno_kernel=ANNO_NONE)
        spb = int(self.options.get("GAT_COUNT_SAMPLES_PER_BLOCK", LIST_SAMPLES_PER_BLOCK))
        return dict(kernel=KERNEL_SEG, staged=self.staged, hits=1 if all_six else 0, patch=0, tracks_per_block=self.tt,
                    samples_per_block=spb, merged_form=0, anno_kernel=self.anno if all_six else ANNO_NONE)

    def expected(self, counters):
        """[counter][track, list] from oracle.counter, summed over the groups as the reference does"""
        from oracle import oracle as O
        key = tuple(counters)
        if key in self._expected:
            return self._expected[key]
        G = self.n_groups
        out, memo = [], {}
        for c in counters:
            dens = c == "nucleotide-density"
            m = np.zeros((self.n_tracks, self.n_lists), dtype=np.float64 if dens else np.int64)
            for t in range(self.n_tracks):
                for l in range(self.n_lists):  # noqa: E741
                    acc = 0.0 if dens else 0
                    for g in range(G):
                        a = self.annos[t * G + g]
                        k = (c, l, g, a.tobytes(), self.ws_nseg[g] if dens else 0)      # (tracks repeat in the merged cases)
                        if k not in memo:
                            memo[k] = O.counter(c, self.lists[l * G + g], a, self.ws_nseg[g])
                        acc += memo[k] if dens else int(memo[k])
                    m[t, l] = acc
            out.append(m)
        self._expected[key] = out
        return out


# ---- the per-base model ---------------------------------------------------------------------------------------
class Masks(object):
    """boolean masks, one entry per base, of a case's lists (made once per list)"""

    def __init__(self, case):
        self.width = case.max_coord() + 1
        assert self.width <= MODEL_MAX + 1
        self._m = {}

    def of(self, a):
        k = a.tobytes()
        if k not in self._m:
            m = np.zeros(self.width, dtype=bool)
            for s, e in zip(a["start"].tolist(), a["end"].tolist()):
                assert not m[s:e].any()
                m[s:e] = True
            run = np.zeros(self.width + 1, dtype=np.int64)
            np.cumsum(m, out=run[1:])
            self._m[k] = (m, run)
        return self._m[k]


def model_counter(masks, name, x, y, ws_nseg):
    """counter `name` of segment list x against track y, from its definition on masks"""
    if name.startswith("annotation-"):
        x, y, name = y, x, name.replace("annotation-", "segment-")
    mx, _ = masks.of(x)
    my, run = masks.of(y)
    if name == "nucleotide-overlap":
        return int(np.count_nonzero(mx & my))
    if name == "nucleotide-density":
        return float(int(np.count_nonzero(mx & my))) / ws_nseg if ws_nseg != 0 else None
    s, e = x["start"].astype(np.int64), x["end"].astype(np.int64)
    if name == "segment-overlap":
        return int(np.count_nonzero(run[e] - run[s] > 0))
    assert name == "segment-midoverlap"
    return int(np.count_nonzero(my[s + (e - s) // 2])) if len(x) else 0


def mid_model_applies(x, y):
    """no segment of x has its midpoint in an interval of y other than the first one that ends behind its start"""
    if len(x) == 0 or len(y) == 0:
        return True
    s, e = x["start"].astype(np.int64), x["end"].astype(np.int64)
    mid = s + (e - s) // 2
    ye, ys = y["end"].astype(np.int64), y["start"].astype(np.int64)
    j_mid = np.searchsorted(ye, mid, side="right")
    inside = (j_mid < len(y)) & (ys[np.minimum(j_mid, len(y) - 1)] <= mid)
    j_first = np.searchsorted(ye, s, side="right")
    return bool(np.all(~inside | (j_mid == j_first)))


def model_expected(case, counters):
    """[counter][track, list] from the mask model, and a boolean array of the same shape: where it applies"""
    G = case.n_groups
    if case.max_coord() > MODEL_MAX:
        return None, [np.zeros((case.n_tracks, case.n_lists), dtype=bool) for _ in counters]
    masks = Masks(case)
    vals, oks, memo = [], [], {}
    for c in counters:
        dens = c == "nucleotide-density"
        m = np.zeros((case.n_tracks, case.n_lists), dtype=np.float64 if dens else np.int64)
        ok = np.ones((case.n_tracks, case.n_lists), dtype=bool)
        for t in range(case.n_tracks):
            for l in range(case.n_lists):  # noqa: E741
                acc = 0.0 if dens else 0
                for g in range(G):
                    x, y = case.lists[l * G + g], case.annos[t * G + g]
                    k = (c, l, g, y.tobytes(), case.ws_nseg[g] if dens else 0)
                    if k not in memo:
                        applies = True
                        if c == "segment-midoverlap":
                            applies = mid_model_applies(x, y)
                        elif c == "annotation-midoverlap":
                            applies = mid_model_applies(y, x)
                        memo[k] = (model_counter(masks, c, x, y, case.ws_nseg[g]), applies)
                    v, applies = memo[k]
                    ok[t, l] &= applies
                    if v is not None:               # (density: only the groups with ws_nseg != 0, left to right)
                        acc += v
                m[t, l] = acc
        vals.append(m)
        oks.append(ok)
    return vals, oks


def swap_roles(case, name, branch):
    """the same geometry with the roles exchanged: the tracks become the lists and the lists the tracks (one group)"""
    assert case.n_groups == 1
    return Case(name, branch, case.annos, case.lists, case.n_tracks, case.n_lists, 1, ws_nseg=case.ws_nseg,
                staged=1, anno=ANNO_IDX)


# ---- generators, each named for the branch it targets ------------------------------------------------------------
def edge_probes(a, b):
    """the probe lists around one interval [a, b): name -> segment list"""
    P = {
        "last base before a": [(a - 1, a)], "first base": [(a, a + 1)], "last base": [(b - 1, b)], "first base behind b": [(b, b + 1)],
        "the interval": [(a, b)], "one base wider": [(a - 1, b + 1)], "one base behind a's base": [(a + 1, a + 2)],
        "bookended at a": [(a - 5, a), (a, a + 3)], "bookended at b": [(b - 3, b), (b, b + 4)],
    }
    for what, m in (("a-1", a - 1), ("a", a), ("b-1", b - 1), ("b", b)):
        for length in (5, 6):
            s = m - length // 2
            P["midpoint %s, length %d" % (what, length)] = [(s, s + length)]
    return P


def edges_of_one_interval(a, b):
    """segs_vs_pairs / seg_vs_anno: `reach` (pe_raw > xs), `mid < pe_raw`, `sk <= mid` and `sk < xe` with xs, xe and the midpoint
    ON a, b - 1 and b.  Track 0 is the lone interval (the {0,0} entry in front and the sentinels behind are its neighbours),
    track 1 has neighbours on both sides, track 2 is the one-base interval [a, a + 1)."""
    assert a >= 8 and b > a
    probes = edge_probes(a, b)
    names = sorted(probes)
    annos = [seg([(a, b)]), seg([(max(0, a - 500), max(1, a - 400)), (a, b), (b + 400, b + 500)]) if a >= 500 else seg([(0, 1), (a, b), (b + 400, b + 500)]),
             seg([(a, a + 1)])]

    def premise(case):
        mids = set()
        for n in names:
            for s, e in probes[n]:
                mids.add(midpoint(s, e))
        assert {a - 1, a, b - 1, b} <= mids
        for what, m in (("a-1", a - 1), ("a", a), ("b-1", b - 1), ("b", b)):
            for length in (5, 6):
                (s, e), = probes["midpoint %s, length %d" % (what, length)]
                assert e - s == length and midpoint(s, e) == m
        assert probes["bookended at a"][0][1] == probes["bookended at a"][1][0] == a
        assert probes["bookended at b"][0][1] == probes["bookended at b"][1][0] == b
        assert len(case.annos[2]) == 1 and case.annos[2]["end"][0] - case.annos[2]["start"][0] == 1
    c = Case("edges[%d,%d)" % (a, b), edges_of_one_interval.__doc__, [seg(probes[n]) for n in names], annos, len(names), 3, 1,
             premise=premise)
    c.probe_names = names
    return c


def cluster(k, far_end, grid_factor=2, far=FAR):
    """segs_vs_pairs' slow test `p2.x < xs`: k one-base intervals two bases apart share ONE grid cell (cell 0, or the last one),
    so a segment starting behind, or inside behind the second, has a third start in front of xs in its own cell; a far interval
    makes max_start -- and with it the cells -- large."""
    span = 2 * (k - 1) + 1
    c0 = far - 2 * (k - 1) if far_end else 0
    starts = [c0 + 2 * i for i in range(k)]
    track = [(s, s + 1) for s in starts]
    track = ([(0, 1)] + track) if far_end else (track + [(far, far + 1)])
    inside = [(c0 + 2 * i, c0 + 2 * i + 2) for i in range(k)]                # starts ON start i: i starts in front of xs
    if far_end:
        behind = [(5, 9), (far + 1, far + 10)]                                # ... all k (and the origin's) in front
        spans = [(c0 - 3, far + 2)]
    else:
        behind = [(starts[-1] + 1, starts[-1] + 10), (far - 3, far + 3)]
        spans = [(0, starts[-1] + 2), (far, far + 1)]
    gaps = [(c0 + 2 * i + 1, c0 + 2 * i + 2) for i in range(k - 1)] + [(starts[-1] + 1, starts[-1] + 2)]   # the bases between them
    # behind the cluster and on to the far interval: all k starts in front of xs AND a base in common (the origin's cluster)
    reach = [(starts[-1] + 1, far + 1)] if not far_end else [(1, 3), (far + 2, far + 5)]
    lists = [seg(inside), seg(behind), seg(spans), seg(gaps), seg(reach)]

    def premise(case):
        y = case.annos[0]
        max_start, longest = int(y["start"][-1]), len(y)
        assert max_start == far and longest == k + 1
        assert span <= min_cell_width(max_start, longest, grid_factor)
        sh, cells = grid_shift(max_start, longest, grid_factor)
        assert (1 << sh) >= min_cell_width(max_start, longest, grid_factor)
        cell = set(s >> sh for s in starts)
        assert cell == ({cells - 1} if far_end else {0})
        assert sum(1 for s in starts if s < behind[-1 if far_end else 0][0]) == k          # every start in front of `behind`
        assert sum(1 for s, e in inside if sum(1 for q in starts if q < s) >= 3) == k - 3
        if not far_end:
            assert sum(1 for q in starts if q < reach[0][0]) == k and reach[0][1] > far
    opts = {"GAT_GRID_FACTOR": str(grid_factor)} if grid_factor != 2 else {}
    return Case("cluster[k=%d,%s,gf=%d]" % (k, "far" if far_end else "origin", grid_factor), cluster.__doc__, lists, [seg(track)],
                5, 1, 1, options=opts, premise=premise)


def few_intervals(m):
    """the {0,0} entry in front of a staged list and the three sentinels behind it ARE the four pairs the look-up reads when a
    list has 0 to 3 intervals; `g < cells - 1` clamps a position beyond the last grid cell"""
    ivs = [(1000, 1100), (3000, 3100), (5000, 5100)][:m]
    xs = [(10, 20), (500, 5600), (6000, 6010), (900000, 900010)]

    def premise(case):
        assert case.max_m() == m
        if m:
            sh, cells = grid_shift(ivs[-1][0], m)
            assert (xs[-1][0] >> sh) > cells - 1                              # beyond the last cell
            assert xs[0][1] <= ivs[0][0] and xs[2][0] >= ivs[-1][1]
            assert xs[1][0] < ivs[0][0] and xs[1][1] > ivs[-1][1]
    return Case("few_intervals[%d]" % m, few_intervals.__doc__, [seg(xs)], [seg(ivs)], 1, 1, 1, staged=1 if m else 0, premise=premise)


def _ladder(n, step, length, start=3):
    return seg([(start + step * i, start + step * i + length) for i in range(n)])


def segment_list_length(n):
    """k_count_seg's one-pass boundary: a list of up to 512 = 64 lanes x kCountXR segments is held in registers, a longer one is
    read pass by pass; 63 / 64 / 65 are the lanes of one round.  No segments at all: the annotation side has no list to index."""
    tracks = [_ladder(410, 25, 7), seg([(100, 200), (5000, 5003), (10250, 10300)])]

    def premise(case):
        assert len(case.lists[0]) == n and case.max_m() == 410
    return Case("segment_list_length[%d]" % n, segment_list_length.__doc__, [_ladder(n, 10, 3)], tracks, 1, 2, 1,
                anno=ANNO_IDX if n else ANNO_PLAIN, premise=premise)


def annotation_list_length(m, lds_entries=None):
    """the staged boundary max_m + 4 <= GAT_COUNT_LDS_ENTRIES: the longest list that still fits LDS, and the first that does not"""
    E = lds_entries or LDS_ENTRIES
    opts = {"GAT_COUNT_LDS_ENTRIES": str(E)} if lds_entries else {}

    def premise(case):
        assert case.max_m() == m and case.staged == (1 if m + 4 <= E else 0)
    return Case("annotation_list_length[%d,E=%d]" % (m, E), annotation_list_length.__doc__, [_ladder(150, 61, 9, start=0)],
                [_ladder(m, 9, 5)], 1, 1, 1, options=opts, staged=1 if m + 4 <= E else 0, premise=premise)


def shrunk_tile():
    """the track tile shrinks to GAT_COUNT_LDS_ENTRIES / (max_m + 4) = 1024 / 304 = 3 tracks: 16 tracks make five tiles of three
    and a last one of one track"""
    tracks = [_ladder(300 - 17 * t, 31 + t, 6 + t) for t in range(16)]

    def premise(case):
        assert case.max_m() == 300 and LDS_ENTRIES // (300 + 4) == 3 and case.n_tracks % 3 == 1
    return Case("shrunk_tile", shrunk_tile.__doc__, [_ladder(200, 47, 11)], tracks, 1, 16, 1, tt=3, premise=premise)


def tiles(n_tracks, n_groups, tpb=None, seed=5):
    """the track tile: a ragged last tile, a track that is empty inside a tile (on every group / on one group), a group that is
    empty for every track, a list without segments in a group, a group whose ws_nseg is 0"""
    rs = np.random.RandomState(seed + 100 * n_tracks + n_groups)

    def rand_list(n, hi=60000):
        st = np.sort(rs.choice(hi // 40, size=n, replace=False)) * 40
        return seg([(int(s), int(s) + int(rs.randint(1, 40))) for s in st])
    empty_track = 2 if n_tracks >= 15 else None
    empty_once = (5, 1) if n_tracks >= 15 and n_groups > 1 else None
    empty_group = 2 if n_groups == 3 else None
    annos = []
    for t in range(n_tracks):
        for g in range(n_groups):
            if t == empty_track or (t, g) == empty_once or g == empty_group:
                annos.append(EMPTY)
            else:
                annos.append(rand_list(int(rs.randint(5, 21))))
    n_lists = 2
    lists = [EMPTY if (l == 1 and g == 0 and n_groups > 1) else rand_list(int(rs.randint(30, 90))) for l in range(n_lists) for g in range(n_groups)]  # noqa: E741
    ws_nseg = [3, 0, 7][:n_groups] if n_groups > 1 else [5]
    tt = min(n_tracks, tpb or TRACKS_PER_BLOCK)

    def premise(case):
        G = n_groups
        if empty_track is not None:
            assert all(len(case.annos[empty_track * G + g]) == 0 for g in range(G))
        if empty_once is not None:
            t, g = empty_once
            assert len(case.annos[t * G + g]) == 0 and any(len(case.annos[t * G + h]) for h in range(G))
        if empty_group is not None:
            assert all(len(case.annos[t * G + empty_group]) == 0 for t in range(n_tracks))
        if G > 1:
            assert 0 in case.ws_nseg and len(case.lists[1 * G + 0]) == 0
        assert 0 < case.max_m() <= 20
    opts = {"GAT_COUNT_TRACKS_PER_BLOCK": str(tpb)} if tpb else {}
    return Case("tiles[T=%d,G=%d,tpb=%s]" % (n_tracks, n_groups, tpb), tiles.__doc__, lists, annos, n_lists, n_tracks, n_groups,
                ws_nseg=ws_nseg, options=opts, tt=tt, premise=premise)


MERGED_LENGTHS = (65535, 65536, 65537, 200000)


def merged(n_tracks, n_lists, block=None, bound1=False, lists_merged=False):
    """k_count_merged: intervals longer than the piece bound (at most 32 768 bases, the 16-bit length) are cut into pieces whose
    overlaps must add up to the interval's; the three fetch forms (GAT_MERGED_BLOCK 8, 2, 1) give the same sums; the same
    interval in every track makes every entry of a scan a hit"""
    ivs, pos = [], 1000
    for length in MERGED_LENGTHS:
        ivs.append((pos, pos + length))
        pos += length + 10
    track = seg(ivs)
    lists = []
    for l in range(n_lists):  # noqa: E741
        xs = [(3 + l, 900 + l)]
        for (s, e) in ivs:
            xs.append((s - 2 + (l % 3), s + 1 + l))                                    # over the interval's start
            for j in (8, 10, 15):                                                   # over where a piece of 2^j bases ends
                xs.append((s + (1 << j) - 1 - (l % 2), s + (1 << j) + 1 + l))
            xs.append((s + 40000, e - 20 - l))                                       # longer than any piece
            xs.append((e - 1 - (l % 2), e + 3))                                      # over its end
        xs.append((pos + 100, pos + 200 + l))
        lists.append(seg(sorted(xs)))
    opts = {}
    if block:
        opts["GAT_MERGED_BLOCK"] = str(block)
    if bound1:
        opts["GAT_MERGED_BOUND"] = "1"
    if lists_merged:
        opts["GAT_COUNT_LISTS_MERGED"] = "1"
    if n_tracks < 4:
        opts["GAT_MERGED_MIN_TRACKS"] = "1"
    takes_merged = n_lists >= 16 or lists_merged

    def premise(case):
        assert [int(e - s) for s, e in zip(track["start"], track["end"])] == list(MERGED_LENGTHS)
        assert all(case.annos[t].tobytes() == track.tobytes() for t in range(n_tracks))
        assert min(MERGED_LENGTHS) > 32768                                           # every interval is cut, whatever the bound
        assert (case.merged is not None) == takes_merged
    return Case("merged[T=%d,L=%d,blk=%s,bound1=%d,knob=%d]" % (n_tracks, n_lists, block, bound1, lists_merged), merged.__doc__,
                lists, [track] * n_tracks, n_lists, n_tracks, 1, options=opts,
                merged=(block or "any") if takes_merged else None, premise=premise)


def annotation_side(n, no_swap=False):
    """k_count_anno_idx indexes the list in LDS -- 2 * (n + 1) * 4 bytes and a grid of at most 2^13 cells -- and falls back to
    k_count_anno when that no longer fits 160 KiB, or under GAT_COUNT_NO_SWAP; from 8 192 segments on the grid's cells clamp at 2^13"""
    lds = 2 * (n + 1) * 4 + ((1 << min(13, max(4, (n).bit_length()))) + 1) * 4
    plain = no_swap or lds + 1024 > 160 * 1024
    tracks = [_ladder(50, 3 * n // 50, 1 + 2 * n // 50 - t, start=t) for t in range(3)]

    def premise(case):
        assert len(case.lists[0]) == n and all(e - s == 1 for s, e in zip(case.lists[0]["start"], case.lists[0]["end"]))
        assert (case.anno == ANNO_PLAIN) == plain
        if n == 9000:
            assert (1 << 13) < n + 1 and not plain                                   # the clamp of lcells
        if n == 20000:
            assert plain and not no_swap
    return Case("annotation_side[%d,no_swap=%d]" % (n, no_swap), annotation_side.__doc__, [_ladder(n, 3, 1)], tracks, 1, 3, 1,
                options={"GAT_COUNT_NO_SWAP": "1"} if no_swap else {}, anno=ANNO_PLAIN if plain else ANNO_IDX, premise=premise)


TOP = (1 << 31) - 1          # the highest end check_list accepts


def highest_coordinates():
    """32-bit positions: ends of 2^31 - 1, midpoints and running lengths beyond 2^30"""
    lists = [seg([(5, 9), (TOP - 1000, TOP - 500), (TOP - 400, TOP)]), seg([(1, TOP)])]
    annos = [seg([(0, 6), (TOP - 700, TOP - 300), (TOP - 1, TOP)]), seg([(7, TOP)]), seg([(TOP - 2, TOP)])]

    def premise(case):
        assert case.max_coord() == TOP and all(check_list(a) is None for a in case.lists + case.annos)
    return Case("highest_coordinates", highest_coordinates.__doc__, lists, annos, 2, 3, 1, premise=premise)


def sum_beyond_32_bits():
    """a group's overlap is a 32-bit sum, the sum over the groups is not: three groups of 2^31 - 1 common bases"""
    lists = [seg([(0, TOP)])] * 3
    annos = [seg([(0, TOP)])] * 3 + [seg([(0, 5), (7, TOP)]), seg([(1, TOP)]), seg([(0, TOP - 1)])]

    def premise(case):
        assert 3 * TOP > 1 << 32
    return Case("sum_beyond_32_bits", sum_beyond_32_bits.__doc__, lists, annos, 1, 2, 3, ws_nseg=[1, 2, 4], premise=premise)


def refused():
    """(segment lists, annotation lists, code): an end of 2^31 is GAT_ERR_ARG on either side"""
    ok = seg([(5, 9)])
    bad = seg([(5, 9), (100, 1 << 31)])
    return [(bad, ok, ERR_ARG), (ok, bad, ERR_ARG)]


def fuzz(seed):
    """seeded mixtures of clusters -- intervals 0, 1 or 2 bases apart -- and very long gaps, on both sides: bookended runs, several
    starts per grid cell, segments over many intervals, and lists from none to a few hundred intervals"""
    rs = np.random.RandomState(7000 + seed)

    def mixture(n_max):
        out, pos = [], int(rs.randint(0, 3000))
        while len(out) < n_max and pos < MODEL_MAX - 70000:
            for _ in range(int(rs.randint(1, 13))):
                length = int(rs.choice([1, 1, 2, 3, int(rs.randint(1, 41)), int(rs.randint(1, 3000))], p=[.25, .15, .15, .15, .25, .05]))
                out.append((pos, pos + length))
                pos += length + int(rs.randint(0, 3))
                if len(out) >= n_max:
                    break
            pos += int(rs.choice([int(rs.randint(3, 50)), int(rs.randint(1000, 60000))]))
        return seg(out)
    n_groups, n_tracks, n_lists = int(rs.randint(1, 4)), int(rs.randint(1, 6)), int(rs.randint(1, 4))
    small = seed % 4 == 0                                                        # (lists that fit a tile of 16 entries too)
    cap = lambda: int(rs.randint(0, 13)) if small else int(rs.choice([0, 3, 40, 200, 400]))  # noqa: E731
    lists = [mixture(int(rs.choice([0, 1, 70, 300, 600]))) for _ in range(n_lists * n_groups)]
    annos = [mixture(cap()) for _ in range(n_tracks * n_groups)]
    ws_nseg = [int(rs.randint(0, 9)) for _ in range(n_groups)]
    c = Case("fuzz[%d]" % seed, fuzz.__doc__, lists, annos, n_lists, n_tracks, n_groups, ws_nseg=ws_nseg)
    c.staged = 1 if 0 < c.max_m() <= LDS_ENTRIES - 4 else 0
    c.tt = tile_tracks(n_tracks, c.max_m(), c.staged)
    c.anno = ANNO_IDX if c.longest_list(n_lists - 1) > 0 else ANNO_PLAIN
    return c


FUZZ_SEEDS = list(range(100))
FUZZ_SETTINGS = {
    "defaults": {},
    "unstaged": {"GAT_COUNT_STAGED": "0"},
    "tile16": {"GAT_COUNT_LDS_ENTRIES": "16", "GAT_GRID_FACTOR": "1"},
}


def fuzz_under(seed, setting):
    c = fuzz(seed)
    c.options = dict(FUZZ_SETTINGS[setting])
    if setting == "unstaged":
        c.staged = 0
    elif setting == "tile16":
        c.staged = 1 if 0 < c.max_m() <= 16 - 4 else 0
    c.tt = tile_tracks(c.n_tracks, c.max_m(), c.staged, int(c.options.get("GAT_COUNT_LDS_ENTRIES", LDS_ENTRIES)))
    c.name = "fuzz[%d,%s]" % (seed, setting)
    return c


def direct_cases():
    """every case of the direct path but the fuzz seeds"""
    out = [edges_of_one_interval(8, 13), edges_of_one_interval(1000, 1010), edges_of_one_interval(4096, 4097)]
    out += [swap_roles(c, "roles_exchanged:" + c.name, "k_count_anno_idx / k_count_anno: " + c.branch) for c in out[:3]]
    out += [cluster(k, far_end) for k in (3, 4, 8, 64) for far_end in (False, True)]
    out += [cluster(8, True, grid_factor=1), cluster(64, False, grid_factor=4)]
    out += [few_intervals(m) for m in (0, 1, 2, 3)]
    out += [segment_list_length(n) for n in (0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025)]
    out += [annotation_list_length(m) for m in (1019, 1020, 1021)]
    out += [annotation_list_length(m, 16) for m in (11, 12, 13)]
    out += [shrunk_tile()]
    out += [tiles(1, 1), tiles(15, 3), tiles(16, 3), tiles(17, 3), tiles(33, 3), tiles(33, 1), tiles(17, 3, tpb=1), tiles(17, 3, tpb=3)]
    out += [merged(17, 16, block=8), merged(17, 16, block=2), merged(17, 16, block=1), merged(17, 16), merged(17, 15),
            merged(17, 1, block=2, lists_merged=True), merged(1, 16, block=1), merged(17, 16, block=2, bound1=True),
            merged(17, 16, block=8, bound1=True), merged(600, 2, block=8, lists_merged=True), merged(600, 2, block=1, bound1=True, lists_merged=True)]
    out += [annotation_side(20000), annotation_side(9000), annotation_side(300, no_swap=True)]
    out += [highest_coordinates(), sum_beyond_32_bits()]
    return out
