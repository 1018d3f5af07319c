"""Units for the local permutation sampler (k_permute_local) and the helpers its tests share: the `units_flat` /
`model_units` of tests/sampler_edges.py for sampler kind 4, and the generators of the GPU tests.  TEST INFRASTRUCTURE ONLY.

The model is tests/local_permutation_model.py, pinned to the reference by its known answers.  A generated unit never
makes the reference raise (free >= 0 in every piece, no coordinate that can leave 2^31 - 1): those shapes are known
answers and have tests of their own.
"""
import random

import local_permutation_model as M
from oracle import oracle as O
from sampler_edges import CountingRandom, as_lists, device_units, model_counts, rand_norm   # noqa: F401
import sampler_edges as E

LOCAL = 4                               # GAT_SAMPLER_LOCAL_PERMUTATION
LDS_LIST = 2048                         # the LDS bound of the kernel's final list and of a piece's lengths / points
SEEDS = [0, 1234, 2 ** 32 - 3]          # test_units_vs_model
N_RANDOM_UNITS, N_SAMPLES = 60, 4


def units_flat(units):
    return E.units_flat(units, LOCAL)


def filter_is_empty(segments, workspace):
    """no segment overlaps the workspace (SegmentList.filter gives an empty list)."""
    return not any(s < we and e > ws for s, e in segments for ws, we in workspace)


def note_events(rng, segments, workspace, stats):
    """one model sample with its events counted in stats; what the model raises is counted under its class name."""
    try:
        out = M.sample(rng, segments, workspace, stats)
    except (ValueError, OverflowError) as e:
        stats[type(e).__name__] = stats.get(type(e).__name__, 0) + 1
        return None
    if out and len(segments) * len(workspace) <= 1 << 16 and filter_is_empty(segments, workspace):
        stats["output_without_filter"] = stats.get("output_without_filter", 0) + 1
    return out


def model_units(flat, seed, s0, s1, stats=None):
    """the model's (sample, unit) lists in gat_sample_units' order and n_draws, the 32-bit words consumed.  Unit u of
    sample s draws from random.seed((seed + s * n_units + u) mod 2^32)."""
    n = int(flat["n_units"])
    segs, ws = O.aslist(flat["segs"]), O.aslist(flat["ws"])
    so, wo = flat["seg_off"], flat["ws_off"]
    lists, st = [], dict(n_draws=0)
    for s in range(s0, s1):
        for u in range(n):
            us, uw = segs[so[u]:so[u + 1]], ws[wo[u]:wo[u + 1]]
            if not us or not uw:
                lists.append([])
                continue
            rng = CountingRandom((seed + s * n + u) & 0xFFFFFFFF)
            lists.append(M.sample(rng, us, uw) if stats is None else note_events(rng, us, uw, stats))
            st["n_draws"] += rng.words
    return lists, st


def _safe(unit):
    """the reference samples the unit without raising, whatever the draws."""
    t = M.unit_tables(*unit)
    return all(free >= 0 and we + free <= M.INT_MAX for _, _, _, we, free in t)


def frag_ws(r, n, start, lens=(1, 1, 2, 5), gaps=(0, 1, 1, 2, 7)):
    """n short pieces from `start`, separated by gaps drawn from `gaps` (0: adjacent pieces)."""
    out, x = [], start
    for _ in range(n):
        ln = r.choice(lens)
        out.append((x, x + ln))
        x += ln + r.choice(gaps)
    return out


def random_units(r, n, fragmented=1.0 / 3):
    """n units; a third with a fragmented workspace of hundreds of pieces.  Segments begin after some workspace (idle
    pieces in front) in some units and the workspace ends before some segments in others."""
    units = []
    while len(units) < n:
        span = r.choice([200, 1000, 5000, 40000])
        lo = r.choice([0, 0, span // 4])
        segs = rand_norm(r, r.randint(1, 40), span, r.choice([1, 5, 50]), start=lo)
        if r.random() < fragmented:
            ws = frag_ws(r, r.randint(100, 400), r.choice([0, lo, span // 2]))
        else:
            ws = rand_norm(r, r.randint(1, 20), span + 100, r.choice([1, 3, 30, 2000]), start=r.choice([0, span // 2]))
        if segs and ws and _safe((segs, ws)):
            units.append((segs, ws))
    return units


def small_piece_unit(r, n_pieces=5000):
    """several thousand active pieces of one or two working segments each: short segments every 10-20 bases, a piece
    per segment or two."""
    segs, ws, x = [], [], 1000
    for _ in range(n_pieces):
        segs.append((x, x + r.choice((1, 2, 3))))
        if r.random() < 0.3:                       # a second segment starting inside the same piece
            segs.append((x + 5, x + 6))
        ws.append((x + 1, x + r.choice((4, 8))))
        x += r.choice((10, 12, 20))
    return segs, ws


def fixed_units():
    """hand-built (name, units), one per branch of k_permute_local."""
    r = random.Random(29)
    big = 2 ** 31
    short = (rand_norm(r, 20, 5000, 50), [(0, 5100)])
    # 2 600 working segments over two pieces (about 1 300 each): 5 200 raw pieces and a final list of some 2 600, beyond
    # the 2 048 of the LDS list -- sorted and merged in the slab
    long_list = (rand_norm(r, 2600, 800_000, 60), [(0, 400_000), (400_001, 900_000)])
    # 2 600 working segments in ONE piece: lengths and points beyond LDS, kept in the unit's slab region
    long_piece = (rand_norm(r, 2600, 900_000, 80), [(0, 1_000_000), (1_000_100, 1_000_200)])
    edges = [
        ([(500, 510)], [(100, 200)]),                                   # empty result, no draw
        ([(10, 20)], [(100, 200)]),                                     # output although filter() is empty
        ([(10, 20)], [(0, 5), (100, 200), (300, 310)]),                 # idle piece first; the segment works for two pieces
        ([(0, 40), (40, 100)], [(0, 100)]),                             # free = 0
        ([(0, 5), (7, 12)], [(0, 12)]),                                 # free = 2: starts and ends on work_end
        ([(0, 10), (20, 31)], [(5, 52)]),                               # free + 1 = 32
        ([(0, 3)], [(1, 36)]),                                          # free + 1 = 34
        ([(10, 300), (400, 700)], [(0, 650)]),                          # wraps
        ([(100 + 10 * i, 103 + 10 * i) for i in range(90)], [(0, 2000), (2000, 2100)]),      # n > 64, adjacent pieces
        ([(0, big // 2), (big // 2 + 5, big - 3000)], [(0, big - 2000)]),                    # near 2^31, free = 1 005
    ]
    return [
        ("long_list", [short, long_list]),
        ("long_piece", [long_piece, short]),
        ("small_pieces", [small_piece_unit(r)]),
        ("edges", edges),
    ]
