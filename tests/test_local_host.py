"""CPU: gat-local's host side -- a row's statistics from the five words against engine.getTwoSidedPValue, numpy.std and
AnnotatorResult on the row of sample values, which rows are written and how, q-values per track, and what is refused."""
import importlib.util
import io
import math
import os
import random

import numpy as np
import pytest

import local_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def script():
    spec = importlib.util.spec_from_file_location("gat_local_cli", os.path.join(ROOT, "scripts", "gat-local.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def words_of(row, obs):
    return M.words(np.array(row, dtype=np.int64).reshape(-1, 1, 1), np.array([[obs]], dtype=np.int64))[0, 0]


def rows_and_observations():
    """integer rows with many ties and zeros, and for each the observed values worth asking: below, at and above the mean,
    below the smallest and above the largest value (idx == l), every value of the row and its neighbours"""
    r = random.Random(11)
    rows = [[5] * 7, [0] * 9, [0, 0, 0, 0, 3], [1], [2, 2, 2, 8, 8, 8], [0, 4]]
    for n in (2, 10, 33, 100):
        for vals in ([0, 0, 0, 1, 2], [0, 7, 7, 7, 20], list(range(6)), [0, 0, 0, 0, 0, 0, 0, 1000]):
            rows.append([r.choice(vals) for _ in range(n)])
    for row in rows:
        mean = sum(row) / len(row)
        cands = set(row) | {v + 1 for v in row} | {max(0, v - 1) for v in row} | {0, int(mean), int(mean) + 1, max(row) + 5}
        if mean == int(mean):
            cands.add(int(mean))
        yield row, sorted(cands)


def test_pvalue_from_two_counts_is_getTwoSidedPValue():
    from gat_amd import engine, local
    n = at_mean = beyond = 0
    for row, cands in rows_and_observations():
        srt = np.sort(np.array(row, dtype=np.float64))
        mean = float(np.mean(srt))
        for obs in cands:
            w = words_of(row, obs)
            expected, _, fold, p = local.bin_statistics(obs, w, len(row))
            assert expected == mean
            assert p == engine.getTwoSidedPValue(srt, mean, float(obs)), (row, obs)
            res = engine.AnnotatorResult("t", "a", "c", obs, row)
            assert (p, fold, expected) == (res.pvalue, res.fold, res.expected), (row, obs)
            n += 1
            at_mean += obs == mean
            beyond += obs > max(row)
    assert n > 100 and at_mean > 3 and beyond > 10


def test_annotator_result_keeps_its_arithmetic():
    """_two_sided calls the lifted function: the values it gave before, on counts given by hand"""
    from gat_amd import engine
    f = engine.twoSidedPValueFromCounts
    assert f(10, 0, True, 10) == 0.1 and f(10, 0, False, 10) == 0.1                  # idx == l
    assert f(3, 2, True, 10) == 0.7 and f(0, 2, True, 10) == 0.9 and f(3, 0, True, 10) == 0.6
    assert f(3, 2, False, 10) == 0.5 and f(0, 0, False, 10) == 0.1 and f(0, 10, False, 10) == 1.0
    res = engine.AnnotatorResult("t", "a", "c", 4, [0, 0, 4, 4, 9])
    assert res.pvalue == f(2, 2, True, 5) == res.getEmpiricalPValue(4.0)


def test_stddev():
    from gat_amd import local
    for row, _ in rows_and_observations():
        sd = local.bin_statistics(0, words_of(row, 0), len(row))[1]
        want = float(np.std(np.array(row, dtype=np.float64)))
        assert abs(sd - want) <= 1e-9 * max(want, 1e-300) or (want == 0 and sd == 0), (row, sd, want)
    # the radicand passes 2^64 (Python integers), and sumsq itself 2^63: it comes back in an int64 and is read as unsigned
    for row in ([2 ** 26] * 500 + [0] * 500, [2 ** 31, 2 ** 31, 0]):
        w = words_of(row, 0)
        assert len(row) * (int(w[2]) % 2 ** 64) > 2 ** 64
        sd = local.bin_statistics(0, w, len(row))[1]
        want = float(np.std(np.array(row, dtype=np.float64)))
        assert abs(sd - want) <= 1e-9 * want, (sd, want)
    assert words_of([2 ** 31, 2 ** 31, 0], 0)[2] < 0


def hand_table():
    from gat_amd import local
    S = 4
    v = np.zeros((S, 2, 5), dtype=np.int64)                  # two annotations, contigs of 3 and 2 bins of 10 bases
    v[:, 0, 1] = [0, 3, 3, 10]
    v[:, 1, 4] = [1, 0, 0, 0]
    v[:, 1, 0] = [2, 2, 2, 2]
    obs = np.zeros((2, 5), dtype=np.int64)
    obs[0, 1], obs[0, 3], obs[1, 0] = 3, 7, 2
    return local.rows("trk", ["A", "B"], ["chr1", "chrX"], [0, 3, 5], 10, obs, M.words(v, obs), S), local


def test_rows_selection_and_format():
    res, local = hand_table()
    # observed > 0 or sum > 0: (A, bin 1), (A, chrX bin 0: observed only), (B, bin 0), (B, chrX bin 1: sampled only)
    assert [(x.annotation, x.contig, x.start, x.end, x.observed, x.samples_with_overlap) for x in res] == [
        ("A", "chr1", 10, 20, 3, 3), ("A", "chrX", 0, 10, 7, 0), ("B", "chr1", 0, 10, 2, 4), ("B", "chrX", 10, 20, 0, 1)]
    a, only_obs, const, only_null = res
    assert (a.expected, a.pvalue) == (4.0, 0.75) and abs(a.stddev - math.sqrt(13.5)) < 1e-12 and a.fold == 4.0 / 5.0
    assert (only_obs.expected, only_obs.stddev, only_obs.fold, only_obs.pvalue) == (0.0, 0.0, 1.0, 0.25)
    assert (const.expected, const.stddev, const.fold, const.pvalue) == (2.0, 0.0, 1.0, 1.0)
    assert (only_null.expected, only_null.fold, only_null.pvalue) == (0.25, 1.0 / 1.25, 0.75)
    local.set_qvalues(res, "bonferroni")
    assert [x.qvalue for x in res] == [1.0, 1.0, 1.0, 1.0]
    local.set_qvalues(res, "none")
    assert str(a) == "trk\tA\tchr1\t10\t20\t3\t4.0000\t3.6742\t0.8000\t-0.3219\t7.5000e-01\t7.5000e-01\t3"
    sink = io.StringIO()
    local.write_results(sink, res, "pvalue")
    lines = sink.getvalue().splitlines()
    assert lines[0].split("\t") == list(local.HEADER) and len(local.HEADER) == 13
    assert [l.split("\t")[10] for l in lines[1:]] == ["2.5000e-01", "7.5000e-01", "7.5000e-01", "1.0000e+00"]
    assert lines[2].split("\t")[1:3] == ["A", "chr1"] and lines[3].split("\t")[1:3] == ["B", "chrX"]    # (ties keep their order)
    sink = io.StringIO()
    local.write_results(sink, res, "annotation")
    assert [l.split("\t")[1:4] for l in sink.getvalue().splitlines()[1:]] == [["A", "chr1", "10"], ["A", "chrX", "0"], ["B", "chr1", "0"],
                                                                            ["B", "chrX", "10"]]
    with pytest.raises(ValueError, match="unknown sort order"):
        local.write_results(io.StringIO(), res, "nothing")


def test_qvalues_per_track():
    from gat_amd import local, stats
    res, _ = hand_table()
    more, _ = hand_table()
    for x in more[:2]:
        x.track = "other"
    family = res + more[:2]
    local.set_qvalues(family, "BH")
    assert [x.qvalue for x in res] == stats.adjustPValues([x.pvalue for x in res], method="BH").tolist()
    assert [x.qvalue for x in more[:2]] == stats.adjustPValues([x.pvalue for x in more[:2]], method="BH").tolist()
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(ValueError, match="qvalue-method"):
            local.set_qvalues(family, bad)


def test_parser_and_what_is_refused():
    import gat_amd
    from gat_amd import local
    mod = script()
    opts, args = mod.buildParser().parse_args([])
    assert args == [] and opts.bin_size == 100000 == local.BIN_SIZE and opts.sampler == "annotator" and opts.qvalue_method == "BH"
    assert opts.num_samples == 1000 and opts.pseudo_count == 1.0
    opts, _ = mod.buildParser().parse_args(["--segments=s.bed", "--annotations=a.bed", "--workspace=w.bed", "--isochores=i.bed",
                                            "--sampler=shift", "--num-samples=20", "--random-seed=4", "--bin-size=500", "--order=track",
                                            "-q", "holm", "--pseudo-count=0.5", "--device=1"])
    assert (opts.segment_files, opts.annotation_files, opts.workspace_files, opts.isochore_files) == (["s.bed"], ["a.bed"], ["w.bed"], ["i.bed"])
    assert (opts.sampler, opts.num_samples, opts.random_seed, opts.bin_size, opts.output_order, opts.qvalue_method, opts.pseudo_count,
            opts.device) == ("shift", 20, 4, 500, "track", "holm", 0.5, 1)
    for name in gat_amd.CLI_SAMPLERS:
        assert mod.buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in local.QVALUE_METHODS:
        assert mod.buildParser().parse_args(["--qvalue-method=%s" % name])[0].qvalue_method == name
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(SystemExit):
            mod.buildParser().parse_args(["--qvalue-method=%s" % bad])
    for argv, what in ((["--conditional=cooccurance"], "conditional"), (["--annotations-to-points=midpoint"], "annotations-to-points"),
                       (["--reference-stream"], "reference-stream")):
        with pytest.raises(NotImplementedError, match=what):
            mod.main(["gat-local.py"] + argv)
    with pytest.raises(NotImplementedError, match="run on the GPU path"):
        local.track_local("t", None, None, None, object(), 10)


def test_too_many_bins_is_refused_before_the_device(monkeypatch):
    """n_tracks * total_bins > 2^27: ValueError that names the way out; nothing reaches the library"""
    from gat_amd import local
    mod = script()
    opts, _ = mod.buildParser().parse_args(["--segments=%s" % os.path.join(CLI, "segments.bed"),
                                            "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
                                            "--workspace=%s" % os.path.join(CLI, "workspace.bed")])
    segments, annotations, workspace = local.build_inputs(opts)
    monkeypatch.setattr(local, "MAX_CELLS", 10)
    monkeypatch.setattr(local, "get_context", lambda: pytest.fail("the device was asked"))
    with pytest.raises(ValueError, match="choose a larger --bin-size"):
        local.run(segments, annotations, workspace, local.make_sampler(opts), 10, bin_size=1, random_seed=1)
    for bad in (0, 2 ** 31 + 1):
        with pytest.raises(ValueError, match="bin_size"):
            local.run(segments, annotations, workspace, local.make_sampler(opts), 10, bin_size=bad, random_seed=1)
    with pytest.raises(ValueError, match="num_samples"):
        local.run(segments, annotations, workspace, local.make_sampler(opts), 0, random_seed=1)
    with pytest.raises(ValueError, match="qvalue-method"):
        local.run(segments, annotations, workspace, local.make_sampler(opts), 10, qvalue_method="storey")
