"""CPU: gat-pairs' host side -- the order of the pairs, a row's statistics from the five words against numpy.mean, numpy.std and
engine.getTwoSidedPValue on the row of sample values, which rows are written and how, q-values per track, and what is refused."""
import importlib.util
import io
import math
import os

import numpy as np
import pytest

import pairs_model as M
from test_local_host import rows_and_observations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def script():
    spec = importlib.util.spec_from_file_location("gat_pairs_cli", os.path.join(ROOT, "scripts", "gat-pairs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("T", [1, 2, 3, 64, 65])
def test_pair_index_is_the_loop(T):
    from gat_amd import pairs
    k = pairs.pair_index(T)
    assert k.shape == (T, T) and k.dtype == np.int64
    n = 0
    for i in range(T):
        for j in range(i, T):
            assert k[i, j] == k[j, i] == n == i * T - i * (i - 1) // 2 + (j - i)
            n += 1
    assert n == T * (T + 1) // 2 and M.pair_list(T) == [(i, j) for i in range(T) for j in range(i, T)]


def test_row_statistics_from_the_words():
    from gat_amd import engine, pairs
    n = 0
    for row, cands in rows_and_observations():
        values = np.array(row, dtype=np.int64).reshape(-1, 1)
        srt = np.sort(np.array(row, dtype=np.float64))
        for obs in cands:
            w = M.words(values, np.array([obs], dtype=np.int64))[0]
            x = pairs.PairResult("t", "a", "b", obs, w, len(row), obs + 1, obs + 2)
            assert x.expected == float(np.mean(srt)) and x.samples_with_hit == sum(1 for v in row if v > 0)
            want_sd = float(np.std(srt))
            assert abs(x.stddev - want_sd) <= 1e-9 * max(want_sd, 1e-300) or (want_sd == 0 and x.stddev == 0)
            assert x.pvalue == engine.getTwoSidedPValue(srt, float(np.mean(srt)), float(obs)), (row, obs)
            res = engine.AnnotatorResult("t", "a", "c", obs, row)
            assert (x.pvalue, x.fold, x.expected) == (res.pvalue, res.fold, res.expected)
            n += 1
    assert n > 100


def hand_table(include_single=False):
    from gat_amd import pairs
    S = 4
    names = ["A", "B", "C"]                                     # pairs: AA AB AC BB BC CC
    v = np.zeros((S, 6), dtype=np.int64)
    v[:, 0] = [4, 5, 5, 6]                                      # AA
    v[:, 1] = [0, 3, 3, 10]                                     # AB
    v[:, 3] = [2, 3, 3, 10]                                     # BB
    v[:, 4] = [1, 0, 0, 0]                                      # BC: sampled only
    v[:, 5] = [1, 0, 0, 0]                                      # CC
    obs = np.array([5, 3, 7, 4, 0, 7], dtype=np.int64)           # AC: observed only
    return pairs.rows("trk", names, obs, M.words(v, obs), S, include_single=include_single), pairs


def test_rows_selection_and_format():
    res, pairs = hand_table()
    assert [(x.annotation_a, x.annotation_b, x.observed, x.samples_with_hit, x.observed_a, x.observed_b) for x in res] == [
        ("A", "B", 3, 3, 5, 4), ("A", "C", 7, 0, 5, 7), ("B", "C", 0, 1, 4, 7)]
    ab, only_obs, only_null = res
    assert (ab.expected, ab.pvalue) == (4.0, 0.75) and abs(ab.stddev - math.sqrt(13.5)) < 1e-12 and ab.fold == 4.0 / 5.0
    assert (only_obs.expected, only_obs.stddev, only_obs.fold, only_obs.pvalue) == (0.0, 0.0, 1.0, 0.25)
    assert (only_null.expected, only_null.fold, only_null.pvalue) == (0.25, 1.0 / 1.25, 0.75)
    pairs.set_qvalues(res, "none")
    assert str(ab) == "trk\tA\tB\t3\t4.0000\t3.6742\t0.8000\t-0.3219\t7.5000e-01\t7.5000e-01\t3\t5\t4"
    single, _ = hand_table(include_single=True)
    assert [(x.annotation_a, x.annotation_b) for x in single] == [("A", "A"), ("A", "B"), ("A", "C"), ("B", "B"), ("B", "C"), ("C", "C")]
    assert [(x.observed, x.observed_a, x.observed_b) for x in single if x.annotation_a == x.annotation_b] == [(5, 5, 5), (4, 4, 4), (7, 7, 7)]
    # a pair without an observed or a sampled hit is no row, single or not
    none = pairs.rows("trk", ["A", "B"], [0, 0, 3], np.zeros((3, 5), dtype=np.int64), 4, include_single=True)
    assert [(x.annotation_a, x.annotation_b) for x in none] == [("B", "B")]
    sink = io.StringIO()
    pairs.write_results(sink, res, "pvalue")
    lines = sink.getvalue().splitlines()
    assert lines[0].split("\t") == list(pairs.HEADER) and len(pairs.HEADER) == 13
    assert lines[0] == ("track\tannotation_a\tannotation_b\tobserved\texpected\tstddev\tfold\tl2fold\tpvalue\tqvalue\tsamples_with_hit\t"
                        "observed_a\tobserved_b")
    assert [l.split("\t")[8] for l in lines[1:]] == ["2.5000e-01", "7.5000e-01", "7.5000e-01"]
    assert [l.split("\t")[1:3] for l in lines[1:]] == [["A", "C"], ["A", "B"], ["B", "C"]]                 # (ties keep the pairs' order)
    sink = io.StringIO()
    pairs.write_results(sink, list(reversed(res)), "track")
    assert [l.split("\t")[1:3] for l in sink.getvalue().splitlines()[1:]] == [["A", "B"], ["A", "C"], ["B", "C"]]
    with pytest.raises(ValueError, match="unknown sort order"):
        pairs.write_results(io.StringIO(), res, "nothing")


def test_qvalues_per_track():
    from gat_amd import pairs, stats
    res, _ = hand_table()
    more, _ = hand_table()
    for x in more[:2]:
        x.track = "other"
    family = res + more[:2]
    pairs.set_qvalues(family, "BH")
    assert [x.qvalue for x in res] == stats.adjustPValues([x.pvalue for x in res], method="BH").tolist()
    assert [x.qvalue for x in more[:2]] == stats.adjustPValues([x.pvalue for x in more[:2]], method="BH").tolist()
    pairs.set_qvalues(res, "bonferroni")
    assert [x.qvalue for x in res] == [1.0, 0.75, 1.0]
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(ValueError, match="qvalue-method"):
            pairs.set_qvalues(family, bad)


def test_parser_and_what_is_refused():
    import gat_amd
    from gat_amd import pairs
    mod = script()
    opts, args = mod.buildParser().parse_args([])
    assert args == [] and opts.sampler == "annotator" and opts.qvalue_method == "BH" and opts.include_single is False
    assert opts.num_samples == 1000 and opts.pseudo_count == 1.0 and not hasattr(opts, "bin_size")
    opts, _ = mod.buildParser().parse_args(["--segments=s.bed", "--annotations=a.bed", "--workspace=w.bed", "--isochores=i.bed",
                                            "--sampler=shift", "--num-samples=20", "--random-seed=4", "--order=fold", "--include-single",
                                            "-q", "holm", "--pseudo-count=0.5", "--device=1"])
    assert (opts.segment_files, opts.annotation_files, opts.workspace_files, opts.isochore_files) == (["s.bed"], ["a.bed"], ["w.bed"], ["i.bed"])
    assert (opts.sampler, opts.num_samples, opts.random_seed, opts.output_order, opts.qvalue_method, opts.pseudo_count, opts.device,
            opts.include_single) == ("shift", 20, 4, "fold", "holm", 0.5, 1, True)
    for name in gat_amd.CLI_SAMPLERS:
        assert mod.buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in pairs.QVALUE_METHODS:
        assert mod.buildParser().parse_args(["--qvalue-method=%s" % name])[0].qvalue_method == name
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(SystemExit):
            mod.buildParser().parse_args(["--qvalue-method=%s" % bad])
    with pytest.raises(SystemExit):
        mod.buildParser().parse_args(["--bin-size=10"])
    for argv, what in ((["--conditional=cooccurance"], "conditional"), (["--annotations-to-points=midpoint"], "annotations-to-points"),
                       (["--reference-stream"], "reference-stream")):
        with pytest.raises(NotImplementedError, match=what):
            mod.main(["gat-pairs.py"] + argv)
    with pytest.raises(NotImplementedError, match="run on the GPU path"):
        pairs.track_pairs("t", None, None, None, object(), 10)


def test_refused_before_the_device(monkeypatch):
    """more tracks than the cap, no samples, an unknown q-value method: ValueError; nothing reaches the library"""
    from gat_amd import pairs
    mod = script()
    opts, _ = mod.buildParser().parse_args(["--segments=%s" % os.path.join(CLI, "segments.bed"),
                                            "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
                                            "--workspace=%s" % os.path.join(CLI, "workspace.bed")])
    segments, annotations, workspace = pairs.build_inputs(opts)
    monkeypatch.setattr(pairs, "get_context", lambda: pytest.fail("the device was asked"))
    with pytest.raises(ValueError, match="num_samples"):
        pairs.run(segments, annotations, workspace, pairs.make_sampler(opts), 0, random_seed=1)
    with pytest.raises(ValueError, match="qvalue-method"):
        pairs.run(segments, annotations, workspace, pairs.make_sampler(opts), 10, qvalue_method="storey")
    monkeypatch.setattr(pairs, "MAX_TRACKS", 2)
    with pytest.raises(ValueError, match="annotation tracks are more than 2"):
        pairs.run(segments, annotations, workspace, pairs.make_sampler(opts), 10, random_seed=1)
