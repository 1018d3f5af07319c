"""SamplerCircular's contract ("k_circular") in plain Python ints and loops, drawing from the
oracle's RandomState as tests/shift_model.py does.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the library's
circular sampler with it, and tests/test_circular_model.py checks it base by base against a brute force.

The reference has no such sampler, so there are no known answers of its own: the contract is what is written here.

  W       the unit's workspace pieces: sorted, disjoint, touching pieces kept apart; Wsum their bases
  linear  a base of piece j at genome position x has the linear position x - (the gaps before it)
  working the segments cut to W, in linear coordinates, pieces that touch there united: n sorted, disjoint,
          non-touching intervals [a, b)
  draw    r = randint(0, Wsum), the only one; none when n == 0 or Wsum == 0
  sample  interval x covers [a_x + r, b_x + r) modulo Wsum, mapped back to the genome and cut at every border of W it
          crosses and at the wrap; nothing is united afterwards; the list is in genome order
"""
import bisect


def workspace_sum(workspace):
    return sum(e - s for s, e in workspace)


def linear_intervals(segments, workspace):
    """the working list in linear workspace coordinates: [(a, b)], sorted, disjoint, non-touching."""
    out = []
    first, before_first = 0, 0                      # the first piece that ends beyond the segment's start, the bases in front
    for s, e in segments:
        while first < len(workspace) and workspace[first][1] <= s:
            before_first += workspace[first][1] - workspace[first][0]
            first += 1
        j, before = first, before_first
        while j < len(workspace) and workspace[j][0] < e:
            ws, we = workspace[j]
            lo, hi = max(s, ws), min(e, we)
            if lo < hi:
                a, b = before + lo - ws, before + hi - ws
                if out and out[-1][1] == a:
                    out[-1] = (out[-1][0], b)
                else:
                    out.append((a, b))
            before += we - ws
            j += 1
    return out


def to_genome(workspace, lo, hi, cum=None):
    """the linear range [lo, hi) of W (0 <= lo < hi <= Wsum) as genome pieces, one per piece of W it reaches into.  cum: the
    bases in front of every piece, when the caller has them."""
    if cum is None:
        cum = bases_in_front(workspace)
    out = []
    j = bisect.bisect_right(cum, lo) - 1            # the last piece beginning at or before lo
    while j < len(workspace) and cum[j] < hi:
        ws, we = workspace[j]
        a, b = max(lo, cum[j]), min(hi, cum[j] + we - ws)
        if a < b:
            out.append((ws + a - cum[j], ws + b - cum[j]))
        j += 1
    return out


def bases_in_front(workspace):
    cum, t = [], 0
    for s, e in workspace:
        cum.append(t)
        t += e - s
    return cum


def rotate(intervals, workspace, r):
    """the linear intervals rotated by r (0 <= r < Wsum), as the genome-ordered list of pieces."""
    wsum = workspace_sum(workspace)
    cum = bases_in_front(workspace)
    out = []
    for a, b in intervals:
        lo, hi = a + r, b + r
        if hi <= wsum:
            parts = [(lo, hi)]
        elif lo >= wsum:
            parts = [(lo - wsum, hi - wsum)]
        else:                                       # cut by the wrap
            parts = [(lo, wsum), (0, hi - wsum)]
        for x, y in parts:
            out += to_genome(workspace, x, y, cum)
    out.sort()                                      # (the pieces are disjoint: genome order)
    return out


def sample(rng, segments, workspace, stats=None):
    """SamplerCircular().sample(segments, workspace) drawing from rng (an oracle RandomState).  stats receives n, wsum
    and r (None when nothing was drawn)."""
    if stats is None:
        stats = {}
    segments = [tuple(x) for x in segments]
    workspace = [tuple(x) for x in workspace]
    iv = linear_intervals(segments, workspace)
    wsum = workspace_sum(workspace)
    stats.update(n=len(iv), wsum=wsum, r=None)
    if not iv or wsum == 0:
        return []
    r = rng.randint(0, wsum)
    stats["r"] = r
    return rotate(iv, workspace, r)


def model_units(flat, seed, s0, s1, info=None):
    """the model's (sample, unit) lists of a flat problem in gat_sample_units' order, and the 32-bit words drawn.  Unit u of
    sample s draws from the stream seeded with (seed + s * n_units + u) mod 2^32.  info, when a list, receives one stats
    dict per (sample, unit)."""
    from oracle import oracle as O
    n = int(flat["n_units"])
    segs, ws = O.aslist(flat["segs"]), O.aslist(flat["ws"])
    so, wo = flat["seg_off"], flat["ws_off"]
    lists, ndraws = [], 0
    for s in range(s0, s1):
        for u in range(n):
            rng = O.RandomState((seed + s * n + u) & 0xFFFFFFFF)
            st = {}
            lists.append(sample(rng, segs[so[u]:so[u + 1]], ws[wo[u]:wo[u + 1]], st))
            ndraws += rng.ndraws
            if info is not None:
                info.append(st)
    return lists, ndraws
