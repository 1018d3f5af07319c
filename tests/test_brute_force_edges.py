"""CPU: the generators of tests/brute_force_edges.py reach what they are for, and everything they make converges --
checked on the model (tests/brute_force_model.py), no device.  tests/test_sampler_brute_force_edges_gpu.py runs the same
calls on the device, so a branch reached here is a branch the GPU tests drive k_brute_force through."""
import pytest

import brute_force_edges as B
import brute_force_model as M


@pytest.fixture(scope="module")
def fuzz():
    """per fuzz seed: the model's lists, statistics and notes of exactly the call test_brute_fuzz[seed] makes."""
    out = []
    for seed in range(B.N_SEEDS):
        flat, call_seed, s0, s1 = B.fuzz_call(seed)
        notes = []
        lists, st = B.model_units(flat, call_seed, s0, s1, notes)
        out.append(dict(flat=flat, lists=lists, st=st, notes=notes))
    return out


@pytest.fixture(scope="module")
def fixed():
    """per fixed case that samples: the model's lists, statistics and notes of the call test_brute_fixed[name] makes."""
    out = {}
    for c in B.fixed_units():
        if c["error"]:
            continue
        flat = B.units_flat(c["units"], **c["params"])
        notes = []
        lists, st = B.model_units(flat, c["seed"], 0, B.FIXED_SAMPLES, notes)
        out[c["name"]] = dict(case=c, flat=flat, lists=lists, st=st, notes=notes)
    return out


def test_every_fuzz_seed_converges(fuzz):
    """all 48 seeds, every (sample, unit) of the samples the GPU test uses: none skipped, none resampled."""
    assert len(fuzz) == B.N_SEEDS == 48
    for seed, f in enumerate(fuzz):
        n = int(f["flat"]["n_units"])
        assert 4 <= n <= 8 and len(f["lists"]) == B.FUZZ_SAMPLES * n
        assert f["st"]["unconverged"] == 0 and None not in f["lists"], seed


def test_fuzz_reach(fuzz):
    def seeds_with(pred):
        return sum(1 for f in fuzz if any(pred(n) for n in f["notes"]))

    for ev in M.EVENTS:                                   # every noted event in at least 6 seeds
        assert seeds_with(lambda n: n[ev] > 0) >= 6, ev
    assert sum(1 for f in fuzz if f["st"]["restarts"] > 0) >= 10
    assert seeds_with(lambda n: len(n["passes"]) > 1 and n["passes"][-1][1]) >= 10      # ... followed by a pass that converges
    assert seeds_with(lambda n: n["words"] > B.MT_N) >= 6                               # a stream across the MT twist
    assert seeds_with(lambda n: n["words"] > 2 * B.MT_N) >= 3
    # hits beyond the first ballot step, lists beyond one and two wave widths and beyond the LDS list
    assert seeds_with(lambda n: any(i >= 64 for i in n["hit_lowest"])) >= 6
    assert seeds_with(lambda n: any(i >= 128 for i in n["hit_lowest"])) >= 3
    lengths = [max(len(l) for l in f["lists"]) for f in fuzz]
    assert sum(64 < x <= 128 for x in lengths) >= 3 and sum(x > 128 for x in lengths) >= 6 and sum(x > B.LDS_MAX for x in lengths) >= 2
    # the parameters
    params = [B.params_of(f["flat"]) for f in fuzz]
    for b in (0, 1, 3, 7):
        assert sum(p["bucket_size"] == b for p in params) >= 2
    for nb in (2, 4):
        assert sum(p["nbuckets"] == nb for p in params) >= 2
    assert sum(p["ntries_inner"] < 10 for p in params) >= 24
    # the shapes: units without segments, with an empty working list, with segments outside the workspace, a workspace
    # from 0, pieces of one base, adjacent pieces
    shapes = [B.units_of(f["flat"]) for f in fuzz]
    assert sum(any(not s for s, _ in u) for u in shapes) >= 2
    assert sum(any(s and not B.unit_caps(B.units_flat([(s, w)]))[0] for s, w in u) for u in shapes) >= 2
    assert sum(any(s and s[-1][0] >= w[-1][1] and B.unit_caps(B.units_flat([(s, w)]))[0] for s, w in u) for u in shapes) >= 6
    assert sum(any(any(a < w[-1][1] < b for a, b in s) for s, w in u) for u in shapes) >= 6      # partly outside
    assert sum(any(w[0][0] == 0 for _, w in u) for u in shapes) >= 6
    assert sum(any(w == [(x, x + 1) for x, _ in w] and len(w) == 1 for _, w in u) for u in shapes) >= 6
    assert sum(any(any(a[1] == b[0] for a, b in zip(w, w[1:])) for _, w in u) for u in shapes) >= 6


def test_fixed_cases_converge_and_reach_their_branch(fixed):
    for name, f in fixed.items():
        assert None not in f["lists"] and f["st"]["unconverged"] == 0, name
    n_of = lambda name: [len(l) for l in fixed[name]["lists"]]                                   # noqa: E731
    small = lambda name: bool(fixed[name]["case"]["knobs"])                                        # noqa: E731
    cap = lambda name, scale=1: B.lds_cap(fixed[name]["flat"], small(name), scale)                 # noqa: E731
    # list lengths: exact, at and beside the wave widths and each launch's LDS capacity
    assert n_of("lengths_lds256") == [63, 64, 65, 127, 128, 129, 255, 256, 257] * B.FIXED_SAMPLES and cap("lengths_lds256") == 256
    assert n_of("lengths_lds64") == [63, 64] * B.FIXED_SAMPLES and cap("lengths_lds64") == 64
    assert n_of("lengths_lds64_plus1") == [63, 65] * B.FIXED_SAMPLES and cap("lengths_lds64_plus1") == 64
    assert cap("lengths_lds64_plus1", 2) == 128
    assert n_of("lengths_lds128") == [127, 128] * B.FIXED_SAMPLES and cap("lengths_lds128") == 128
    assert n_of("nonworking_overflow") == [129, 128] * B.FIXED_SAMPLES and cap("nonworking_overflow") == 128
    assert cap("nonworking_overflow", 2) == 256 and not small("nonworking_overflow")
    assert n_of("lengths_lds192") == [191, 192] * B.FIXED_SAMPLES and cap("lengths_lds192") == 192
    assert n_of("lengths_lds192_plus1") == [193] * B.FIXED_SAMPLES and cap("lengths_lds192_plus1") == 192
    for name, f in fixed.items():
        # `retried` is exactly: some list is longer than its unit's region at the first layout
        caps = B.unit_caps(f["flat"], small(name)) * B.FIXED_SAMPLES
        assert f["case"]["retried"] == any(len(l) > c for l, c in zip(f["lists"], caps)), name
    # a list at least 4 times the working list, no knob
    segs, ws = fixed["nonworking_overflow"]["case"]["units"][0]
    assert 129 >= 4 * sum(1 for s, e in segs if s < ws[-1][1])
    # the cases that wait for an event
    for name in ("hit_at_63", "hit_at_64", "hit_in_slab", "touching_both", "slab_pass_then_lds_pass", "lds_pass_then_slab_pass",
                 "remaining_alone", "geometry_near_zero", "long_stream"):
        assert B.fixed_reach(fixed[name]["case"], fixed[name]["notes"]), name
        if name.startswith("hit") or name.endswith("pass"):
            assert cap(name) == B.LDS_MAX
    assert 63 in [i for n in fixed["hit_at_63"]["notes"] for i in n["hit_only"]]
    assert 64 in [i for n in fixed["hit_at_64"]["notes"] for i in n["hit_only"]]
    assert max(i for n in fixed["hit_in_slab"]["notes"] for i in n["hit_only"]) >= B.LDS_MAX
    # (remaining_alone: with nothing hit, such a draw is accepted unless overlap > remaining rejects it)
    assert all(n["words"] > 2 * B.MT_N for n in fixed["long_stream"]["notes"])


def test_sum_cases_are_the_known_answers():
    """the two shapes whose segments.sum() is near 2^31 are known answers, and the reference raised for every seed."""
    kats = M.load_kats()
    for c in B.fixed_units():
        if not c["error"]:
            continue
        mine = [k for k in kats if k["segments"] == c["units"][0][0] and k["workspace"] == c["units"][0][1]]
        assert len(mine) == 6 and all(k["error"] == "ValueError" and k["params"] == B.DEFAULT for k in mine), c["name"]
    big = [c for c in B.fixed_units() if c["name"] == "sum_near_2_31"][0]
    assert sum(e - s for s, e in big["units"][0][0]) == 2 ** 31 - 996


def test_lds_cap_mirrors_the_launch():
    """cap_for: n + n/4 + 96 in whole 64s (n/2 + 8 under GAT_TEST_SMALL_CAPS) of min(segments.sum(), 2 * len(segments));
    no region below 128 without the knob, so lds_cap 64 needs it."""
    assert B.cap_for(1) == 128 and B.cap_for(26) == 128 and B.cap_for(27) == 192 and B.cap_for(256) == 448
    assert B.cap_for(64, True) == 64 and B.cap_for(113, True) == 64 and B.cap_for(114, True) == 128
    assert B.lds_cap(B.units_flat([B.ones(300)])) == 256 and B.lds_cap(B.units_flat([([], [(0, 5)])])) == 64
