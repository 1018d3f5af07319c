"""The overlap-count stage on the device, kernel by kernel: every case of tests/count_cases.py through gat_count_lists -- all six
counters in one call, and the nucleotide pair alone (which is what lets k_count_merged run) -- compared with oracle.counter as
exact integers (density: the same double, bit for bit), and after every call gat_count_last_launch must name the kernel, the
tile and the annotation-side kernel the case was built for.  k_count_swap and the PATCH variants exist only behind the
sampler: small problems through Problem.sample_and_count against oracle.run_samples, every route asserted the same way.
The premises of the cases, and that the per-base model agrees with the oracle, are test_count_cases_model.py's (CPU)."""
import collections

import numpy as np
import pytest

import count_cases as K
from gat_amd import _lib, problem, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = K.direct_cases()
SEGMENT_SIDE = K.COUNTERS[:4]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _count_and_check(ctx, case, counters):
    lists, list_off, annos, anno_off = case.flat()
    got = ctx.count_lists(counters, lists, list_off, case.n_lists, annos, anno_off, case.n_tracks, case.ws_nseg, case.n_groups)
    report = ctx.count_report()
    want = case.expected(counters)
    for k, c in enumerate(counters):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
        bad = np.argwhere(_bits(got[k]) != _bits(want[k]))
        assert len(bad) == 0, (case.name, c, "track, list", bad[0].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    exp = case.report(counters)
    if exp["merged_form"] == "any":
        assert report["merged_form"] in (8, 2, 1), report
        exp = dict(exp, merged_form=report["merged_form"])
    assert report == exp, (case.name, counters)
    return got


def _run_direct(ctx, monkeypatch, case):
    for key, value in case.options.items():
        monkeypatch.setitem(ctx.options, key, value)
    _count_and_check(ctx, case, K.COUNTERS)
    _count_and_check(ctx, case, K.NUCLEOTIDE)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_direct_case(ctx, monkeypatch, case):
    _run_direct(ctx, monkeypatch, case)


_FUZZ = {}


@pytest.mark.parametrize("setting", sorted(K.FUZZ_SETTINGS))
def test_fuzz_seeds(ctx, monkeypatch, setting):
    """all 100 seeds under the defaults, GAT_COUNT_STAGED=0, and a tile of 16 entries with a coarse grid: each equals the
    oracle, so they equal each other; the report says whether the seed's lists were staged"""
    for key, value in K.FUZZ_SETTINGS[setting].items():
        monkeypatch.setitem(ctx.options, key, value)
    staged = 0
    for seed in K.FUZZ_SEEDS:
        base = _FUZZ.setdefault(seed, K.fuzz(seed))
        case = K.fuzz_under(seed, setting)
        case._expected = base._expected                      # (the oracle's values: once per seed)
        _count_and_check(ctx, case, K.COUNTERS)
        _count_and_check(ctx, case, K.NUCLEOTIDE)
        staged += case.staged
    if setting == "unstaged":
        assert staged == 0
    else:
        assert 10 <= staged <= len(K.FUZZ_SEEDS) - (10 if setting == "tile16" else 0)


def test_end_of_2_31_is_refused(ctx):
    for lists, annos, code in K.refused():
        with pytest.raises(ValueError) as e:
            ctx.count_lists(K.COUNTERS, lists, [0, len(lists)], 1, annos, [0, len(annos)], 1, [1], 1)
        assert "error %d:" % code in str(e.value) and code == K.ERR_ARG


def test_no_list_launches_nothing(ctx):
    case = K.few_intervals(2)
    _count_and_check(ctx, case, K.COUNTERS)
    assert ctx.count_report()["kernel"] == K.KERNEL_SEG
    got = ctx.count_lists(K.COUNTERS, K.EMPTY, [0], 0, case.annos[0], [0, 2], 1, [1], 1)
    assert all(g.shape == (1, 0) for g in got)
    assert set(ctx.count_report().values()) == {0}


# ---- behind the sampler ------------------------------------------------------------------------------------------
def _problem(seed, n_contigs, n_segs, n_tracks, n_intervals, isochores=False):
    """a small problem of the kind test_hip_parity._random_problem makes, with the sizes that pick the count route given"""
    rs = np.random.RandomState(seed)
    contigs = collections.OrderedDict(("c%d" % i, int(rs.randint(60000, 300000))) for i in range(n_contigs))
    segs = synthetic.random_segments(contigs, n_segs, 60, int(rs.randint(1 << 30)))
    annos = [("t%d" % t, synthetic.random_segments(contigs, n_intervals + 3 * t, int(rs.randint(50, 2000)), int(rs.randint(1 << 30))))
             for t in range(n_tracks)]
    ws = synthetic.workspace_ungapped(contigs, pieces=int(rs.randint(1, 4)), gap=2000)
    iso = synthetic.isochores_blocks(contigs, nclasses=2, block=int(rs.randint(8000, 40000))) if isochores else None
    return problem.flatten_arrays(segs, annos, ws, iso)


_ORACLE = {}


def _sampled(ctx, monkeypatch, key, flat, counters, S, options, expect):
    """sample_and_count of samples [3, 3 + S) under `options` equals the oracle; the report holds `expect`"""
    okey = (key, tuple(counters), S)
    if okey not in _ORACLE:
        _ORACLE[okey] = O.run_samples(flat, counters, 900, 1, 3, 3 + S)[0]
    want = _ORACLE[okey]
    with monkeypatch.context() as m:
        for k, v in options.items():
            m.setitem(ctx.options, k, v)
        P = _lib.Problem(ctx, flat)
        try:
            got = P.sample_and_count(counters, 900, 3, 3 + S)
            report = ctx.count_report()
        finally:
            P.close()
    for k, c in enumerate(counters):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (key, c, options)
    for field, value in expect.items():
        assert report[field] == value, (key, options, field, report)
    return report


SAMPLES = (5, 70)


@pytest.mark.parametrize("S", SAMPLES)
def test_sampled_swap_by_its_own_rule(ctx, monkeypatch, S):
    """sampled lists more than three times the annotation lists: k_count_swap; the same problem under GAT_COUNT_NO_SWAP: k_count_seg"""
    flat = _problem(11, 2, 500, 2, 24)
    n_contigs, n_tracks = int(flat["n_contigs"]), int(flat["n_tracks"])
    avg_n = (int(flat["seg_off"][-1])) / n_contigs
    avg_m = int(flat["anno_off"][-1]) / (n_contigs * n_tracks)
    assert avg_m > 0 and avg_n > 3 * avg_m and n_tracks < 4                        # its own rule; no merged index
    _sampled(ctx, monkeypatch, "swap", flat, K.NUCLEOTIDE, S, {}, dict(kernel=K.KERNEL_SWAP, merged_form=0, anno_kernel=0))
    _sampled(ctx, monkeypatch, "swap", flat, K.NUCLEOTIDE, S, {"GAT_COUNT_NO_SWAP": "1"},
             dict(kernel=K.KERNEL_SEG, hits=0, staged=1, anno_kernel=0))
    # (with the segment counters beside them the rule does not apply: k_count_seg with hits; all six: the annotation side too)
    _sampled(ctx, monkeypatch, "swap", flat, SEGMENT_SIDE, S, {}, dict(kernel=K.KERNEL_SEG, hits=1, anno_kernel=0))
    _sampled(ctx, monkeypatch, "swap", flat, K.COUNTERS, S, {}, dict(kernel=K.KERNEL_SEG, hits=1, patch=0, anno_kernel=K.ANNO_IDX))
    _sampled(ctx, monkeypatch, "swap", flat, K.COUNTERS, S, {"GAT_COUNT_NO_SWAP": "1"},
             dict(kernel=K.KERNEL_SEG, hits=1, patch=0, anno_kernel=K.ANNO_PLAIN))


@pytest.mark.parametrize("S", SAMPLES)
def test_sampled_patch_and_final_lists(ctx, monkeypatch, S):
    """counts alone: k_count_seg<.., PATCH> reads (merged list, k_tail's record); GAT_COUNT_FINAL_LISTS: the final lists"""
    flat = _problem(12, 3, 240, 3, 150)
    for counters, hits in ((SEGMENT_SIDE, 1), (K.NUCLEOTIDE, 0)):
        _sampled(ctx, monkeypatch, "patch", flat, counters, S, {}, dict(kernel=K.KERNEL_SEG, patch=1, hits=hits, staged=1))
        _sampled(ctx, monkeypatch, "patch", flat, counters, S, {"GAT_COUNT_FINAL_LISTS": "1"},
                 dict(kernel=K.KERNEL_SEG, patch=0, hits=hits, staged=1))
        _sampled(ctx, monkeypatch, "patch", flat, counters, S, {"GAT_COUNT_STAGED": "0"}, dict(kernel=K.KERNEL_SEG, patch=1, hits=hits, staged=0))
        _sampled(ctx, monkeypatch, "patch", flat, counters, S, {"GAT_COUNT_STAGED": "0", "GAT_COUNT_FINAL_LISTS": "1"},
                 dict(kernel=K.KERNEL_SEG, patch=0, hits=hits, staged=0))


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("spb", (1, 3))
def test_sampled_samples_per_block(ctx, monkeypatch, S, spb):
    """GAT_COUNT_SAMPLES_PER_BLOCK: a wave per sample and idle waves (1), a ragged last chunk (3 of 5 and of 70)"""
    flat = _problem(12, 3, 240, 3, 150)
    _sampled(ctx, monkeypatch, "patch", flat, SEGMENT_SIDE, S, {"GAT_COUNT_SAMPLES_PER_BLOCK": str(spb)},
             dict(kernel=K.KERNEL_SEG, samples_per_block=spb, hits=1))
    _sampled(ctx, monkeypatch, "patch", flat, SEGMENT_SIDE, S, {}, dict(kernel=K.KERNEL_SEG, samples_per_block=8))


@pytest.mark.parametrize("isochores", (False, True))
@pytest.mark.parametrize("spb", (1, 3, 64))
def test_sampled_merged_samples_per_block(ctx, monkeypatch, spb, isochores):
    """GAT_MERGED_SAMPLES_PER_BLOCK with 5 samples: one sample a workgroup, 3 + 2, and a group larger than the batch"""
    flat = _problem(13, 3, 240, 5, 150, isochores=isochores)
    key = "merged-iso" if isochores else "merged"
    r = _sampled(ctx, monkeypatch, key, flat, K.NUCLEOTIDE, 5, {"GAT_MERGED_SAMPLES_PER_BLOCK": str(spb)},
                 dict(kernel=K.KERNEL_MERGED, samples_per_block=min(spb, 5), staged=0, hits=0, anno_kernel=0))
    assert r["merged_form"] in (8, 2, 1)
    for block in (8, 2, 1):
        _sampled(ctx, monkeypatch, key, flat, K.NUCLEOTIDE, 5, {"GAT_MERGED_SAMPLES_PER_BLOCK": str(spb), "GAT_MERGED_BLOCK": str(block)},
                 dict(kernel=K.KERNEL_MERGED, merged_form=block))


@pytest.mark.parametrize("S", SAMPLES)
def test_sampled_track_tile_of_three(ctx, monkeypatch, S):
    """GAT_COUNT_TRACKS_PER_BLOCK=3 with 7 tracks: tiles of 3, 3 and 1"""
    flat = _problem(14, 2, 200, 7, 120)
    _sampled(ctx, monkeypatch, "tile3", flat, SEGMENT_SIDE, S, {"GAT_COUNT_TRACKS_PER_BLOCK": "3"},
             dict(kernel=K.KERNEL_SEG, tracks_per_block=3, staged=1, hits=1))
    _sampled(ctx, monkeypatch, "tile3", flat, SEGMENT_SIDE, S, {}, dict(kernel=K.KERNEL_SEG, tracks_per_block=7, staged=1, hits=1))
