"""Problems of the gat_sample_coverage tests (tests/test_coverage_gpu.py).  TEST INFRASTRUCTURE ONLY.

Unit problems (one contig per unit, no annotations: sampler_edges.units_flat) for every sampler (SIX: the six samplers the name
is from, and SamplerCircular's three problems, tests/circular_cases.py), the hand-built problem of the
window-edge test, the one whose bins pass 2^32, and what the tests need of a problem: its contigs' workspace extents.
"""
import random

import numpy as np

import brute_force_edges as BF
import circular_cases as CIRC
import local_permutation_edges as LP
import sampler_edges as E
from gat_amd import problem, synthetic

ANNOTATOR, SEGMENTS = 0, 1
BIN_SIZES = (1, 7, 64, 1000, 1 << 20)
MAX_BINS = 40000                        # bins per contig in the six-sampler test: some twenty k_coverage windows at the default 1 920


def roomy_units(seed, max_len=40):
    """units whose segments (lengths 1..max_len) take a small part of a workspace of a few pieces"""
    r = random.Random(0xC0FE + seed)
    units = []
    for n in (1, 7, 40, 150):
        span = 60 * max_len * n + 500
        segs = E.rand_norm(r, n, span, max_len)
        cut = sorted(r.sample(range(100, span - 100), 4))
        ws = [(0, cut[0]), (cut[0] + 7, cut[1]), (cut[2], cut[3]), (cut[3], span)]
        units.append((segs, ws))
    return units


def unit_problem(name):
    if name == "annotator":
        return E.units_flat(roomy_units(1), ANNOTATOR)
    if name == "segments":
        return E.units_flat(roomy_units(2), SEGMENTS)
    if name == "shift":
        units, radius, extension = E.shift_edge_units(3)
        return E.units_flat(units, E.SHIFT, radius, extension)
    if name == "global-permutation":
        return E.units_flat(E.perm_edge_units(5), E.PERM)
    if name == "local-permutation":
        return LP.units_flat(LP.random_units(random.Random(5), 10))
    if name == "brute-force":                      # (a case of the brute-force fuzz: it converges for the test's seed and samples)
        units, params = BF.edge_units(8)
        return BF.units_flat(units, **params)
    raise KeyError(name)


def genome_problem(sampler, isochores):
    _, cfg = synthetic.small_genome()
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], cfg["isochores"] if isochores else None)
    flat["sampler"] = sampler
    if sampler == E.SHIFT:
        flat["shift_radius"], flat["shift_extension"] = 2.0, 0
    return flat


SIX = {
    "annotator-units": lambda: unit_problem("annotator"),
    "segments-units": lambda: unit_problem("segments"),
    "shift-units": lambda: unit_problem("shift"),
    "global-permutation-units": lambda: unit_problem("global-permutation"),
    "local-permutation-units": lambda: unit_problem("local-permutation"),
    "brute-force-units": lambda: unit_problem("brute-force"),
    "annotator-genome": lambda: genome_problem(ANNOTATOR, False),
    "annotator-genome-isochores": lambda: genome_problem(ANNOTATOR, True),       # the contig lists: k_contig's slab
    "segments-genome": lambda: genome_problem(SEGMENTS, False),                  # neither sorted nor disjoint: the scan
    "segments-genome-isochores": lambda: genome_problem(SEGMENTS, True),
    "shift-genome-isochores": lambda: genome_problem(E.SHIFT, True),
    "global-permutation-genome-isochores": lambda: genome_problem(E.PERM, True),
    "circular-units": lambda: CIRC.units_flat(CIRC.consumer_units()),            # touching pieces, lists longer than the unit
    "circular-genome": lambda: genome_problem(CIRC.CIRCULAR, False),
    "circular-genome-isochores": lambda: genome_problem(CIRC.CIRCULAR, True),    # k_contig merges the touching pieces
}
CIRCULAR_NAMES = ("circular-units", "circular-genome", "circular-genome-isochores")


def extents(flat):
    """per contig of the problem: the largest workspace end of its units"""
    ext = np.zeros(int(flat["n_contigs"]), dtype=np.int64)
    for u, c in enumerate(flat["unit_contig"]):
        w = flat["ws"][flat["ws_off"][u]:flat["ws_off"][u + 1]]
        if c >= 0 and len(w):
            ext[c] = max(ext[c], int(w["end"].max()))
    return ext


def bins_for(flat, bin_size, cap=MAX_BINS):
    """ceil(extent / bin_size) bins per contig, at most cap + 7 * contig: what lies beyond shows in `outside`"""
    ext = extents(flat)
    return np.minimum((ext + bin_size - 1) // bin_size, cap + 7 * np.arange(len(ext))).astype(np.int64)


# ---- window and chunk edges: bins of one base, windows of 64 ------------------------------------------------------------
WINDOW = 64
WINDOW_BINS = (0, 1, 63, 64, 65, 129, 129, 3)


def window_units():
    """a contig per entry of WINDOW_BINS.  The last one's workspace begins far beyond its three bins: everything it samples
    is `outside`; the 129-bin contigs hold segments longer than a window, one of them of 300 bases in a workspace of 700."""
    small = [(1, 2), (5, 8), (11, 12), (20, 30), (33, 34), (40, 41), (45, 47)]
    return [
        ([(5, 9), (20, 30)], [(0, 50)]),
        ([(5, 9), (20, 30)], [(0, 50)]),
        ([(1, 4), (10, 30), (40, 41)], [(0, 63)]),
        ([(1, 4), (10, 30), (40, 41)], [(0, 64)]),
        ([(1, 4), (10, 30), (40, 41), (50, 52)], [(0, 65)]),
        (small + [(50, 120)], [(0, 129)]),
        ([(10 * i, 10 * i + 1 + i % 3) for i in range(20)] + [(250, 550), (560, 650)], [(0, 700)]),
        ([(1005, 1009), (1020, 1030)], [(1000, 1200)]),
    ]


def window_reach(seg, off, n_contigs=len(WINDOW_BINS)):
    """what the lists of a Problem.sample of the window problem reach: a segment starting on a window edge, one ending on
    one, one crossing an edge, one touching three windows, and whether the last contig's lists lie beyond its bins"""
    got = dict(starts_on_edge=False, ends_on_edge=False, crosses=False, three_windows=False, beyond=True)
    for l in range(len(off) - 1):
        c = l % n_contigs
        ext = WINDOW_BINS[c]
        for s, e in zip(seg["start"][off[l]:off[l + 1]].tolist(), seg["end"][off[l]:off[l + 1]].tolist()):
            if c == n_contigs - 1:
                got["beyond"] &= s >= ext
            if ext <= WINDOW:
                continue
            e = min(e, ext)
            if e <= s:
                continue
            got["starts_on_edge"] |= s > 0 and s % WINDOW == 0
            got["ends_on_edge"] |= e % WINDOW == 0 and e < ext
            got["crosses"] |= (e - 1) // WINDOW > s // WINDOW
            got["three_windows"] |= (e - 1) // WINDOW >= s // WINDOW + 2
    return got


# ---- sums beyond 2^32 ----------------------------------------------------------------------------------------------------
BIG_BIN = 1 << 24
BIG_SAMPLES = 400


def big_units():
    """SamplerSegments places every one of five segments of 3 * 2^24 + 7 bases in a workspace of sixteen bins of 2^24: a
    sample adds about 2^24 bases to a bin, most of them through bins covered whole; 400 samples pass 2^32"""
    ln = 3 * BIG_BIN + 7
    return [([(i * (ln + 5), i * (ln + 5) + ln) for i in range(5)], [(0, 16 * BIG_BIN)])]


WINDOW_SEED, WINDOW_SAMPLES = 3, 9      # nine samples from this seed reach every entry of window_reach, under both samplers
