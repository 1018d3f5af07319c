"""CPU: the units of tests/circular_cases.py give lists with the properties the consumers' GPU tests are there for.  Asserted
on tests/circular_model.py alone, for the seed and the samples those tests draw: the GPU tests then assert only equality."""
import circular_cases as CIRC
import circular_model as M

S = CIRC.SAMPLES


def lists_of(units):
    """[sample][unit] -> the model's list, and the stats beside it"""
    info = []
    lists, _ = M.model_units(CIRC.units_flat(units), CIRC.SEED, 0, S, info)
    n = len(units)
    return [lists[s * n:(s + 1) * n] for s in range(S)], [info[s * n:(s + 1) * n] for s in range(S)]


def test_units_are_what_their_names_say():
    units = CIRC.consumer_units()
    assert len(units) == 12 and units[CIRC.EDGE] == (CIRC.EDGE_SEGS, CIRC.EDGE_WS)
    flat = CIRC.units_flat(units)
    assert flat["n_contigs"] == 12 and (flat["unit_contig"] >= 0).all()          # (every unit is a contig: MISSED too)
    n_iv = [len(M.linear_intervals(s, w)) for s, w in units]
    assert n_iv[CIRC.FILLED] == 1 and M.workspace_sum(units[CIRC.FILLED][1]) == units[CIRC.FILLED][1][0][1] - units[CIRC.FILLED][1][0][0]
    assert n_iv[CIRC.WAVE_65] == 65 and n_iv[CIRC.MISSED] == 0 and M.workspace_sum(units[CIRC.WSUM_ONE][1]) == 1
    ws = units[CIRC.CRUMBS][1]
    assert len(ws) > 200 and all(1 <= b - a <= 5 for a, b in ws) and sum(1 for x, y in zip(ws, ws[1:]) if x[1] == y[0]) > 50
    assert all(x[1] <= y[0] for s, w in units for x, y in zip(w, w[1:]))         # sorted, disjoint: touching ones kept apart


def test_consumer_lists_have_the_four_properties():
    units = CIRC.consumer_units()
    lists, info = lists_of(units)
    n_iv = [len(M.linear_intervals(s, w)) for s, w in units]
    every = [(s, u, lists[s][u]) for s in range(S) for u in range(len(units))]
    # touching pieces kept apart -- in the one-piece unit too, where only the wrap can make them
    assert any(x[1] == y[0] for _, _, l in every for x, y in zip(l, l[1:]))
    assert any(len(l) == 2 and l[0][1] == l[1][0] for s, u, l in every if u == CIRC.FILLED)
    # more pieces than the unit has intervals, by far
    assert any(len(l) > n_iv[u] for _, u, l in every)
    assert max(len(l) for _, u, l in every if u == CIRC.CRUMBS) > 20 * n_iv[CIRC.CRUMBS]
    # a wrapped piece first: an interval cut by the wrap, its head at the workspace's first base
    wrapped = [(s, u) for s, u, l in every if l and info[s][u]["r"] and l[0][0] == units[u][1][0][0]
               and any(a + info[s][u]["r"] < info[s][u]["wsum"] < b + info[s][u]["r"] for a, b in M.linear_intervals(*units[u]))]
    assert len({u for _, u in wrapped}) >= 3
    # an empty list beside full ones, and the unit that draws nothing
    assert all(lists[s][CIRC.MISSED] == [] and all(lists[s][u] for u in range(len(units)) if u != CIRC.MISSED) for s in range(S))
    assert all(lists[s][CIRC.WSUM_ONE] == [(7, 8)] and info[s][CIRC.WSUM_ONE]["r"] == 0 for s in range(S))
    # every list is sorted and disjoint, and no two samples of a drawing unit agree by accident everywhere
    assert all(x[0] < x[1] <= y[0] for _, _, l in every for x, y in zip(l, l[1:]))
    assert len({tuple(lists[s][CIRC.CRUMBS]) for s in range(S)}) == S


def test_wide_lists_cross_the_sign_bit():
    units = CIRC.wide_units()
    assert 2 <= len(units) <= 3
    for segs, ws in units:
        assert ws[0][0] < CIRC.TWO_31 < ws[-1][1] and any(a < CIRC.TWO_31 for a, b in segs) and any(b > CIRC.TWO_31 for a, b in segs)
    assert max(w[-1][1] for _, w in units) == CIRC.TOP == 2 ** 32 - 1
    lists, info = lists_of(units)
    every = [l for s in range(S) for l in lists[s]]
    assert all(every)
    both = [l for l in every if l[0][1] <= CIRC.TWO_31 and l[-1][0] >= CIRC.TWO_31]
    assert len(both) > S                                                                  # pieces on both sides of 2^31 in one list
    assert any(a < CIRC.TWO_31 < b for l in every for a, b in l)                          # ... and a piece across it
    assert any(b > 2 ** 32 - 100 for l in every for a, b in l) and any(b == CIRC.TOP for l in every for a, b in l)
    assert any(x[1] == y[0] for l in every for x, y in zip(l, l[1:]))
    assert len({st["r"] for row in info for st in row}) > 2 * S


def test_model_sample_is_the_layout_of_problem_sample():
    """contig lists: the units of a contig one after the other, united where the keys carry isochores.  In the genome problem
    no unit piece happens to touch another unit's; in the dense one they do, and the contig lists unite them"""
    import coverage_cases as CC
    problems = [(name, CC.SIX[name]) for name in CC.CIRCULAR_NAMES] + [("dense-isochores", CIRC.dense_isochore_problem)]
    for name, make in problems:
        flat = make()
        assert int(flat["sampler"]) == CIRC.CIRCULAR
        seg, off = CIRC.model_sample(flat, CIRC.SEED, 0, S)
        useg, uoff = CIRC.model_sample(flat, CIRC.SEED, 0, S, unit_level=True)
        assert len(off) == S * int(flat["n_contigs"]) + 1 and len(uoff) == S * int(flat["n_units"]) + 1
        total = lambda a: int((a["end"].astype("int64") - a["start"].astype("int64")).sum())       # noqa: E731
        assert total(seg) == total(useg) > 0
        if name.endswith("isochores"):
            assert int(flat["merge_contigs"]) == 1 and flat["n_units"] > flat["n_contigs"]
            assert (len(seg) < len(useg)) == (name == "dense-isochores")
            assert all(seg["end"][i] < seg["start"][i + 1] for l in range(len(off) - 1) for i in range(off[l], off[l + 1] - 1))
        else:
            assert int(flat["merge_contigs"]) == 0 and seg.tolist() == useg.tolist()
