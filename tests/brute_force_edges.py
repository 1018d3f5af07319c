"""Edge-case units for the brute-force sampler (k_brute_force) and the helpers its tests share: the `units_flat` /
`model_units` of tests/sampler_edges.py for sampler kind 5, the launch's LDS capacity, and the generators of the GPU tests.
TEST INFRASTRUCTURE ONLY.

The model is tests/brute_force_model.py, pinned to the reference by its known answers; its notes (new_notes) say which
branches a (sample, unit) took.  tests/test_brute_force_edges.py checks on the model that the generators reach what they
claim and that everything converges; tests/test_sampler_brute_force_edges_gpu.py runs the same cases on the device.

What the launch allows (gat_prep_units.h: cap_for, base_cap_for; gat_prep.hip: layout_slab; gat_mi355.hip: enqueue_brute_force): a unit's slab region
holds cap = cap_for(min(segments.sum(), 2 * len(segments))) entries, doubled by every overflow retry, and the LDS list
lds_cap = max(64, min(largest cap, 256)).  So lds_cap < 256 means that NO unit's region is larger than lds_cap: a list
can reach lds_cap exactly (n == cap) there, and the acceptance behind it is an overflow, repeated with doubled regions
and a larger lds_cap.  Accepted entries live in the slab (index >= lds_cap) only under lds_cap == 256.
"""
import random

import brute_force_model as M
import sampler_edges as E
from oracle import oracle as O
from sampler_edges import as_lists, device_units, model_counts   # noqa: F401

BRUTE = 5                               # GAT_SAMPLER_BRUTE_FORCE
LDS_MAX = 256                           # gat_brute_force.h: kBruteLdsCap
MT_N = E.MT_N
N_SEEDS = 48
FUZZ_SAMPLES = 4
DEFAULT = dict(bucket_size=1, nbuckets=100000, ntries_inner=100, ntries_outer=10)


def units_flat(units, bucket_size=1, nbuckets=100000, ntries_inner=0, ntries_outer=0):
    """ntries 0: the reference's 100 / 10."""
    flat = E.units_flat(units, BRUTE)
    flat.update(bucket_size=bucket_size, nbuckets=nbuckets, brute_ntries_inner=ntries_inner, brute_ntries_outer=ntries_outer)
    return flat


def units_of(flat):
    segs, ws = O.aslist(flat["segs"]), O.aslist(flat["ws"])
    so, wo = flat["seg_off"], flat["ws_off"]
    return [(segs[so[u]:so[u + 1]], ws[wo[u]:wo[u + 1]]) for u in range(int(flat["n_units"]))]


def params_of(flat):
    return dict(bucket_size=int(flat.get("bucket_size", 1)), nbuckets=int(flat.get("nbuckets", 100000)),
                ntries_inner=int(flat.get("brute_ntries_inner", 0)) or 100,
                ntries_outer=int(flat.get("brute_ntries_outer", 0)) or 10)


def model_units(flat, seed, s0, s1, notes=None):
    """the model's (sample, unit) lists in gat_sample_units' order (None: not converged) and the call's statistics
    (n_draws, restarts, placed, tries, unconverged).  notes, when a list, receives one brute_force_model.new_notes()
    dict per (sample, unit)."""
    st = {}
    if notes is not None:
        st["notes"] = notes
    lists = M.model_units(units_of(flat), seed, s0, s1, stats=st, **params_of(flat))
    return lists, st


def check_stats(st, mst):
    """the library's statistics of a call against the model's."""
    assert st["n_draws"] == mst["n_draws"], (st["n_draws"], mst["n_draws"])
    assert st["n_restarts"] == mst["restarts"], (st["n_restarts"], mst["restarts"])
    assert st["n_placed"] == mst["placed"] and st["n_unsuccessful"] == mst["tries"]
    assert st["n_unconverged"] == 0 == mst["unconverged"]


def cap_for(n, small_caps=False):
    c = n // 2 + 8 if small_caps else n + n // 4 + 96
    return (c + 63) // 64 * 64


def unit_caps(flat, small_caps=False, cap_scale=1):
    """the slab entries of every active unit's region (0: the unit is not launched)."""
    caps = []
    for segs, ws in units_of(flat):
        if not segs or not ws or not len(O.filter(segs, ws)):
            caps.append(0)
            continue
        total = M.i32(sum(e - s for s, e in segs))
        caps.append(cap_for(min(max(total, 0), 2 * len(segs)), small_caps) * cap_scale)
    return caps


def lds_cap(flat, small_caps=False, cap_scale=1):
    """the accepted segments k_brute_force keeps in LDS in a launch of this problem: max(64, min(max_unit_cap, 256))
    (small_caps: under GAT_TEST_SMALL_CAPS; cap_scale: 2^(overflow retries so far))."""
    return max(64, min(max(unit_caps(flat, small_caps, cap_scale) + [0]), LDS_MAX))


# ------------------------------------------------------------------------------------------------ the fuzz generator
BUCKETS = (1, 0, 3, 7)
# (ntries_inner, ntries_outer): the reference's, and inner counts small enough that passes run out of tries -- with enough
# passes that every (sample, unit) converges all the same (tests/test_brute_force_edges.py asserts it)
TRIES = ((0, 0), (6, 60), (4, 200), (3, 400))


def seed_params(seed):
    """bucket sizes 1, 0, 3, 7 in turn; nbuckets 2 and 4 in a quarter of the seeds each; the tries in turn."""
    nb = (100000, 2, 100000, 4)[(seed // 4) % 4]
    inner, outer = TRIES[(seed // 2) % 4]
    return dict(bucket_size=BUCKETS[seed % 4], nbuckets=nb, ntries_inner=inner, ntries_outer=outer)


def _max_len(bucket_size, nbuckets):
    """the longest segment length getLengthDistribution takes: ceil(length / bucket) < nbuckets."""
    if nbuckets == 2:
        return max(1, bucket_size)
    if nbuckets == 4:
        return 3 * max(1, bucket_size)
    return 12


def _pieces(r, n, start, lens, gaps):
    out, x = [], start
    for _ in range(n):
        ln = r.choice(lens)
        out.append((x, x + ln))
        x += ln + r.choice(gaps)
    return out


def _segs_in(r, n, lo, hi, lens, one=True):
    """n separated segments with lengths from `lens` starting in [lo, hi); a segment of the shortest length first (the
    last bases of a pass can then be placed)."""
    step = max(lens) + 1
    starts = sorted(r.sample(range(lo, hi, step), min(n, len(range(lo, hi, step)))))
    segs = [(s, s + r.choice(lens)) for s in starts]
    if one and segs:
        segs[0] = (segs[0][0], segs[0][0] + min(lens))
    return segs


def _unit(r, lmax):
    lens = sorted({1, min(2, lmax), min(3, lmax), lmax, max(1, lmax // 2)})
    kind = r.choice(("zero", "zero", "frag", "frag", "close", "close", "one_base", "outside", "outside", "idle", "dense"))
    if kind == "zero":              # the workspace starts at 0 and the segments are longer than the first piece's offset
        ws = [(0, r.randint(20, 80))] + _pieces(r, r.randint(0, 3), r.randint(90, 120), (30, 50), (0, 1, 5))
        return _segs_in(r, r.randint(3, 8), 0, ws[-1][1], lens), ws
    if kind == "frag":              # pieces of 1-2 bases, adjacent, 1 apart or closer than a length
        ws = _pieces(r, r.randint(40, 160), r.choice((0, 3, 500)), (1, 1, 2), (0, 1, 1, 2, 5))
        return _segs_in(r, r.randint(2, 6), ws[0][0], ws[-1][1], lens), ws
    if kind == "close":             # pieces of tens of bases, adjacent or closer together than a segment's length
        ws = _pieces(r, r.randint(2, 8), r.choice((0, 7, 1000)), (15, 30, 60), (0, 0, 1, 2, max(1, lmax - 1)))
        return _segs_in(r, r.randint(4, 14), ws[0][0], ws[-1][1], lens), ws
    if kind == "one_base":          # a single piece of one base, segments of one base
        x = r.choice((0, 1, 77))
        return [(x, x + 1)], [(x, x + 1)]
    if kind == "outside":           # segments partly or wholly outside the workspace: they count for `remaining`
        ws = [(200, 200 + r.randint(150, 400))]
        segs = _segs_in(r, r.randint(2, 5), 210, ws[0][1] - 20, lens)
        if segs[-1][1] < ws[0][1] - 1:                                     # one base inside, the rest (lengths > 1) outside
            segs += [(ws[0][1] - 1, ws[0][1] - 1 + max(lens))]
        segs += _segs_in(r, r.randint(1, 6), ws[0][1] + 50, ws[0][1] + 400, lens, one=False)     # wholly outside
        return sorted(segs), ws
    if kind == "idle":              # an empty working list (no draw), or no segments at all (the unit is skipped)
        return ([(5000, 5003)] if r.random() < 0.5 else []), [(0, 100)]
    # dozens to a few hundred short segments in one piece a few times their bases: hits at high indices, long streams
    n = r.choice((70, 130, 200, 280))
    span = n * max(lens) * r.choice((3, 5))
    return _segs_in(r, n, 10, 10 + span - 2 * max(lens), lens), [(r.choice((0, 10)), 10 + span)]


def edge_units(seed):
    """(units, params) of brute-force case `seed`: the seed's parameters (seed_params) and 4-8 units from the menu, with
    segment lengths the seed's histogram takes and few enough bases for the workspace."""
    r = random.Random(0xB2F0 + seed)
    params = seed_params(seed)
    lmax = _max_len(params["bucket_size"], params["nbuckets"])
    units = []
    while len(units) < 4 + seed % 5:
        segs, ws = _unit(r, lmax)
        working = O.aslist(O.filter(segs, ws)) if segs else []
        # (segments.sum() small against the workspace, so that the unit converges: a quarter of its bases at the most --
        #  twice that under bucket sizes 3 and 7, which draw lengths of up to twice the segments')
        if len(ws) > 1 and 4 * max(1, params["bucket_size"]) * sum(e - s for s, e in segs) > sum(e - s for s, e in ws):
            continue
        if working:
            try:
                O.length_distribution(working, params["bucket_size"], params["nbuckets"])
            except ValueError:
                continue
        units.append((segs, ws))
    return units, params


def fuzz_call(seed):
    """(flat, stream seed, first sample, last sample + 1) of fuzz case `seed`: 4 samples from a seed-dependent base."""
    units, params = edge_units(seed)
    return units_flat(units, **params), 3000 + 15485863 * seed, 2 + seed % 7, 2 + seed % 7 + FUZZ_SAMPLES


# ------------------------------------------------------------------------------------------------ the fixed cases
FIXED_SAMPLES = 3


def ones(n, x0=0, spread=40):
    """n segments of one base in one piece of spread * n bases: a list of exactly n, hits are rare."""
    return [(x0 + 5 + spread * i, x0 + 6 + spread * i) for i in range(n)], [(x0, x0 + spread * n + 10)]


def ones_and_outside(total, n_work, x0=0):
    """n_work working segments of one base and one segment outside the workspace that brings segments.sum() to `total`:
    lists of exactly `total` one-base segments from a unit of n_work + 1 -- the region is sized by 2 * (n_work + 1)."""
    segs, ws = ones(n_work, x0, spread=200)
    far = ws[0][1] + 1000
    return segs + [(far, far + total - n_work)], ws


def _two_lengths(n, a, b):
    """n segments of length a and n of length b, alternating, in two adjacent pieces and a third one near by."""
    step = b + 3
    segs = [(10 + step * i, 10 + step * i + (a if i % 2 else b)) for i in range(2 * n)]
    end = 10 + step * 2 * n + 40
    return segs, [(0, end // 2), (end // 2, end), (end + 3, end + 3 + end // 3)]


def fixed_units():
    """hand-built cases, one per branch of k_brute_force: dicts of name, units, params, seed (the call's; samples
    [0, FIXED_SAMPLES)), knobs (context options of the call), retried (the call repeats a batch with doubled regions) and
    error (the reference raises for every sample).  The seeds of the cases that wait for an event were found on the model;
    tests/test_brute_force_edges.py asserts from the model's notes that each case reaches its branch."""
    def case(name, units, seed=99, knobs=None, retried=False, error=False, **params):
        return dict(name=name, units=units, params=dict(DEFAULT, **params), seed=seed, knobs=knobs or {}, retried=retried,
                    error=error)

    small = {"GAT_TEST_SMALL_CAPS": "1"}
    dense = ([(2 * i, 2 * i + 1) for i in range(300)], [(0, 1200)])          # 300 one-base segments, hits up to one draw in four
    pairs = ([(5 * i, 5 * i + 2 + i % 2) for i in range(120)], [(0, 900)])   # lengths 2 and 3, dense: touching on both sides
    mixed = _two_lengths(100, 2, 30)                                         # lists of 256 +- 20
    big = 2 ** 30
    return [
        # list lengths across the wave widths and the LDS capacity, lds_cap 256 (the largest region holds 448): 256 fills
        # LDS, 257 puts one entry into the slab and sorts there
        case("lengths_lds256", [ones(n, 100 * k) for k, n in enumerate((63, 64, 65, 127, 128, 129, 255, 256, 257))]),
        # lds_cap 64 (every region 64 entries, GAT_TEST_SMALL_CAPS): 63 and 64 == lds_cap == the region
        case("lengths_lds64", [ones(63), ones(64)], knobs=small),
        # ... and 65: the 65th acceptance overflows, the batch is repeated with lds_cap 128
        case("lengths_lds64_plus1", [ones(63), ones(65)], knobs=small, retried=True),
        # lds_cap 128 without a knob: regions of 128 (6 segments), lists of 127 and 128 == lds_cap -- 25 times the working list
        case("lengths_lds128", [ones_and_outside(127, 5), ones_and_outside(128, 5)]),
        # ... and 129: the overflow path without GAT_TEST_SMALL_CAPS, repeated with lds_cap 256
        case("nonworking_overflow", [ones_and_outside(129, 5), ones_and_outside(128, 5)], retried=True),
        # lds_cap 192 (30 segments: regions of 192), lists of 191 and 192; and 193, repeated
        case("lengths_lds192", [ones_and_outside(191, 29), ones_and_outside(192, 29)]),
        case("lengths_lds192_plus1", [ones_and_outside(193, 29)], retried=True),
        # a rejection whose only hitting entry is number 63 (the first ballot step's last lane), 64 (the second step's first),
        # and one in the slab
        case("hit_at_63", [dense], seed=SEEDS["hit_at_63"]),
        case("hit_at_64", [dense], seed=SEEDS["hit_at_64"]),
        case("hit_in_slab", [dense], seed=SEEDS["hit_in_slab"]),
        # an accepted segment between two accepted ones, touching both
        case("touching_both", [pairs], seed=SEEDS["touching_both"]),
        # a pass that grows into the slab and runs out of tries, then a pass that converges within LDS; and the reverse
        case("slab_pass_then_lds_pass", [mixed], seed=SEEDS["slab_pass_then_lds_pass"], ntries_inner=8, ntries_outer=40),
        case("lds_pass_then_slab_pass", [mixed], seed=SEEDS["lds_pass_then_slab_pass"], ntries_inner=8, ntries_outer=40),
        # draws of 20 bases rejected when fewer remain, nothing hit
        case("remaining_alone", [([(100 * i, 100 * i + 20) for i in range(3)] + [(400 + 10 * i, 401 + 10 * i) for i in range(5)],
                                  [(0, 5000)])]),
        # the workspace from 0, pieces adjacent and 2 apart, segments of 5-12: q < 0, overlaps smaller than the length,
        # sampling_start at the previous piece's end
        case("geometry_near_zero", [([(3, 15), (20, 25), (40, 49), (52, 53)], [(0, 30), (30, 50), (52, 70)])]),
        # segments.sum() = 2^31 - 996 and 2^30 - 990 over a workspace of 100 bases: the reference raises
        case("sum_near_2_31", [([(10, 20), (1000, big), (big + 5, 2 * big - 1)], [(0, 100)])], error=True),
        case("sum_beyond_workspace", [([(10, 20), (1000, big)], [(0, 100)])], error=True),
        # 600 one-base segments: more than 2 x 624 words in every (sample, unit)
        case("long_stream", [([(2 * i, 2 * i + 1) for i in range(600)], [(0, 2400)])]),
    ]


# the call seeds of the cases that wait for an event (found on the model: find_seed)
SEEDS = {"hit_at_63": 1, "hit_at_64": 1, "hit_in_slab": 1, "touching_both": 1, "slab_pass_then_lds_pass": 6,
         "lds_pass_then_slab_pass": 1}


def fixed_reach(case, notes):
    """whether the notes of the case's (sample, unit)s show the branch the case is named for."""
    name = case["name"]
    passes = [n["passes"] for n in notes]
    if name == "hit_at_63":
        return any(63 in n["hit_only"] for n in notes)
    if name == "hit_at_64":
        return any(64 in n["hit_only"] for n in notes)
    if name == "hit_in_slab":
        return any(i >= LDS_MAX for n in notes for i in n["hit_only"])
    if name == "touching_both":
        return any(n["touching_both"] for n in notes)
    if name == "slab_pass_then_lds_pass":
        return any(len(p) >= 2 and p[-2][0] > LDS_MAX and not p[-2][1] and p[-1][0] <= LDS_MAX and p[-1][1] for p in passes)
    if name == "lds_pass_then_slab_pass":
        return any(len(p) >= 2 and p[-2][0] <= LDS_MAX and not p[-2][1] and p[-1][0] > LDS_MAX and p[-1][1] for p in passes)
    if name == "remaining_alone":
        return any(n["rej_remaining_only"] for n in notes)
    if name == "geometry_near_zero":
        return all(sum(n[k] for n in notes) > 0 for k in ("q_negative", "partial_overlap", "start_at_prev_end"))
    if name == "long_stream":
        return all(n["words"] > 2 * MT_N for n in notes)
    raise KeyError(name)


def find_seed(name, first=1, n=2000):
    """the first call seed from `first` under which fixed case `name` reaches its branch (how SEEDS was made)."""
    case = [c for c in fixed_units() if c["name"] == name][0]
    flat = units_flat(case["units"], **case["params"])
    for seed in range(first, first + n):
        notes = []
        lists, _ = model_units(flat, seed, 0, FIXED_SAMPLES, notes)
        if None not in lists and fixed_reach(case, notes):
            return seed
    return None
