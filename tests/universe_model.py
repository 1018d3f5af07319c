"""SamplerUniverse's contract ("k_universe") in plain Python ints and loops, drawing from the oracle's
RandomState as tests/circular_model.py does.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the library's universe
sampler with it, and tests/test_universe_model.py proves its draw uniform by enumeration.

The reference has no such sampler, so there are no known answers of its own: the contract is what is written here.

  W       the unit's workspace pieces: sorted, disjoint, touching pieces kept apart; m = |W|.  They are the universe
  k       the pieces of W that share at least one base with a segment of the unit (a segment over two pieces hits two)
  sample  k pieces of W chosen uniformly without replacement, each whole, in genome order: always exactly k intervals
  draw    Floyd's algorithm on the smaller side: c = k if 2k <= m else m - k; for j = m - c .. m - 1: t = randint(0, j + 1),
          mark j if t is marked, else t.  The marked pieces are the sample if 2k <= m, else the unmarked ones.  k = 0, k = m
          and m = 0 draw nothing
"""


def hits(segments, workspace):
    """k: one merge walk of the (normalized) segments against the pieces."""
    k = j = 0
    for s, e in segments:
        while j < len(workspace) and workspace[j][1] <= s:
            j += 1
        while j < len(workspace) and workspace[j][0] < e:
            k += 1
            j += 1
    return k


def smaller_side(k, m):
    """(c, invert)"""
    return (k, False) if 2 * k <= m else (m - k, True)


def floyd(draw, m, c):
    """the c marks among range(m); draw(j) stands for randint(0, j + 1)."""
    marked = set()
    for j in range(m - c, m):
        t = draw(j)
        marked.add(j if t in marked else t)
    return marked


def choose(rng, k, m):
    """the sorted indices of the k chosen pieces"""
    c, invert = smaller_side(k, m)
    marked = floyd(lambda j: rng.randint(0, j + 1), m, c)
    return [h for h in range(m) if (h in marked) != invert]


def sample(rng, segments, workspace, stats=None):
    """SamplerUniverse().sample(segments, workspace) drawing from rng (an oracle RandomState).  stats receives k, m, c
    and invert."""
    if stats is None:
        stats = {}
    segments = [tuple(x) for x in segments]
    workspace = [tuple(x) for x in workspace]
    m = len(workspace)
    k = hits(segments, workspace)
    c, invert = smaller_side(k, m)
    stats.update(k=k, m=m, c=c, invert=invert)
    if k == 0:
        return []
    return [workspace[h] for h in choose(rng, k, m)]


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
