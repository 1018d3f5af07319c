"""CPU: the edge generators of tests/sampler_edges.py reach what they are for -- checked on the models
(tests/shift_model.py, tests/permutation_model.py), no device.  tests/test_sampler_edges_gpu.py runs the same cases on
the device, so a branch reached here is a branch the GPU tests drive the kernels through."""
import permutation_model as PM
import sampler_edges as E

SHIFT_SEEDS = list(range(48))
PERM_SEEDS = list(range(48))


def _shift_reach(units, radius, extension):
    flat = E.units_flat(units, E.SHIFT, radius, extension)
    info = []
    lists, _ = E.model_units(flat, 1, 0, 1, info)
    cap = E.shift_lds_cap(flat)
    return dict(out_max=max(map(len, lists)),
                over_cap=max(i.get("raw_pieces_max", 0) for i in info) > cap,
                over_cap_small_work=cap < 512 and max(i.get("raw_pieces_max", 0) for i in info) > cap,
                fill_all_max=max(i.get("fill_all_max", 0) for i in info),
                words_max=max(i.get("words", 0) for i in info),
                empty=sum(i.get("empty_windows", 0) for i in info))


def test_shift_generators_reach_their_branches():
    seen = [_shift_reach(*E.shift_edge_units(seed)) for seed in SHIFT_SEEDS]
    fixed = {name: _shift_reach(u, rad, ext) for name, u, rad, ext in E.shift_fixed_units()}
    for pool in (seen, list(fixed.values())):
        assert any(x["out_max"] > E.LDS_LIST for x in pool)          # an output list beyond the LDS buffer
        assert any(x["over_cap_small_work"] for x in pool)           # the slab normalize with a small max_work
        assert any(x["fill_all_max"] > 64 for x in pool)             # a window taken whole, more than one lane round
        assert any(x["words_max"] > E.MT_N for x in pool)            # a stream across the MT twist
        assert any(x["empty"] > 0 for x in pool)                     # empty windows
    assert sum(x["over_cap"] for x in seen) >= 3 and sum(x["fill_all_max"] > 64 for x in seen) >= 6
    assert sum(x["words_max"] > E.MT_N for x in seen) >= 10
    # each fixed unit reaches its own branch
    assert fixed["slab_normalize"]["over_cap_small_work"] and fixed["slab_normalize"]["out_max"] > E.LDS_LIST
    assert fixed["slab_normalize_mixed"]["over_cap"] and not fixed["slab_normalize_mixed"]["over_cap_small_work"]
    assert fixed["fill_all_lanes"]["fill_all_max"] > 64
    assert fixed["extension_one"]["empty"] > 0 and fixed["extension_one"]["out_max"] == 0
    assert fixed["zero_area"]["empty"] == 3
    assert fixed["long_stream"]["words_max"] > 2 * E.MT_N


def test_shift_window_ends_on_piece_ends():
    """extension 20 around midpoints on multiples of 10, adjacent pieces (0,10),(10,20),..: the window's ends fall on
    piece ends, the pieces truncated to nothing are dropped, and adjacent pieces stay apart in the window."""
    import shift_model as SM
    _, units, radius, extension = [x for x in E.shift_fixed_units() if x[0] == "window_on_piece_ends"][0]
    segs, ws = units[0]
    for s, e in segs:
        w = SM.window(ws, s, e, radius, extension)
        mid = s + (e - s) // 2
        assert w[0][0] == mid - 10 and w[-1][1] == mid + 10 and len(w) == 2, (s, e, w)


def _perm_reach(units):
    flat = E.units_flat(units, E.PERM)
    info = []
    E.model_units(flat, 1, 0, 1, info)
    tables = [PM.unit_tables(s, w) for s, w in units]
    return dict(sizes={len(t[0]) for t in tables if t}, frees={t[2] for t in tables if t},
                straddles=sum(i.get("straddles", 0) for i in info),
                all_head=any(i.get("tail", 1) == 0 and i.get("head", 0) > 0 for i in info),
                all_tail=any(i.get("head", 1) == 0 and i.get("tail", 0) > 0 for i in info),
                split=any(i.get("head", 0) + i.get("tail", 0) > 2 * len(t[0]) for i, t in zip(info, tables) if t),
                words_max=max(i.get("words", 0) for i in info))


def test_perm_generators_reach_their_branches():
    seen = [_perm_reach(E.perm_edge_units(seed)) for seed in PERM_SEEDS]
    fixed = {name: _perm_reach(u) for name, u in E.perm_fixed_units()}
    for pool in (seen, list(fixed.values())):
        sizes = set().union(*(x["sizes"] for x in pool))
        frees = set().union(*(x["frees"] for x in pool))
        assert {1, 63, 64, 65, 129}.issubset(sizes), sorted(sizes)
        assert 2048 in sizes and 2049 in sizes
        assert 0 in frees                                            # _randbelow(1)
        assert any(f + 1 >= 4 and (f + 1) & f == 0 for f in frees)   # free + 1 = 2^k
        assert any(f + 2 >= 4 and (f + 2) & (f + 1) == 0 for f in frees)   # free + 1 = 2^k - 1
        assert any(f >= 1 << 24 for f in frees)
        assert sum(x["straddles"] for x in pool) > 0                 # a segment across the wrap
        assert any(x["all_tail"] for x in pool)                      # every piece before the wrap
        assert any(x["split"] for x in pool)                         # segments cut into many pieces by W
        assert any(x["words_max"] > E.MT_N for x in pool)
    assert sum(x["straddles"] for x in seen) >= 10
    assert fixed["lds_2048"]["sizes"] == {2048} and fixed["slab_2049"]["sizes"] == {2049}
    assert {2048, 2049, 1, 5, 30} == fixed["lds_slab_mixed"]["sizes"]
    assert fixed["wave_widths"]["sizes"] == {1, 63, 64, 65, 128, 129}
    assert 0 in fixed["free_edges"]["frees"] and fixed["fine_w"]["split"]


def test_perm_unit_free_is_exact():
    """perm_unit's W holds exactly `free` bases beyond the working segments, whatever the shape."""
    import random
    r = random.Random(4)
    for n, f in ((1, 0), (64, 1), (65, 255), (10, 1 << 24), (129, 4094)):
        for frag in (False, True) if f <= 6000 else (False,):
            segs, ws = E.perm_unit(r, n, f, frag=frag)
            lengths, _, free = PM.unit_tables(segs, ws)
            assert free == f and len(lengths) == n, (n, f, frag)
