"""CPU: gat-reldist's host side -- the reference points derived from the annotation tracks (the three point choices, tracks
without two points on a contig, the offsets over the problem's contigs), what is refused, and the table: every bin a row, the
reldist columns, the three summary rows, the area row's scaling, the q-value families, the orders."""
import importlib.util
import io
import os

import numpy as np
import pytest

import reldist_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")

# (the workspace of tests/golden/cli holds chrA .. chrD from 12000 on: what lies outside it is cut away with the annotations)
BED = """\
track name=one
chrA\t20000\t20100
chrA\t20050\t20200
chrA\t30000\t30001
chrB\t15000\t15003
track name=two
chrA\t100\t200
chrB\t15000\t15002
chrZ\t5\t9
chrZ\t50\t90
track name=three
chrC\t20000\t20010
chrC\t20010\t20020
chrC\t20030\t20041
"""


def script():
    spec = importlib.util.spec_from_file_location("gat_reldist_cli", os.path.join(ROOT, "scripts", "gat-reldist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(tmp_path, extra=()):
    from gat_amd import reldist
    bed = tmp_path / "annotations.bed"
    bed.write_text(BED)
    opts, _ = script().buildParser().parse_args(["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % bed,
                                                 "--workspace=%s" % os.path.join(CLI, "workspace.bed")] + list(extra))
    return reldist.build_inputs(opts) + (opts,)


def test_points(tmp_path):
    """an interval gives one point; overlapping intervals are one interval first (the tracks are normalized), adjacent ones stay
    two; a track without two points on any of the contigs is left out; the offsets are track-major over the contigs given"""
    from gat_amd import reldist
    segments, annotations, workspace, _ = inputs(tmp_path)
    assert list(annotations.tracks) == ["one", "two", "three"]
    want = {"midpoint": [15001, 20100, 30000, 20005, 20015, 20035], "start": [15000, 20000, 30000, 20000, 20010, 20030],
            "end": [15002, 20199, 30000, 20009, 20019, 20040]}
    for point in reldist.ANNOTATION_POINTS:
        names, pos, off, totals = reldist.point_arrays(annotations, ["chrB", "chrA", "chrC"], point)
        assert names == ["one", "three"] and totals == [3, 3] and pos.dtype == np.uint32 and off.dtype == np.int64
        assert pos.tolist() == want[point] and off.tolist() == [0, 1, 3, 3, 3, 3, 6]
    # `two` has one point on chrB and nothing else inside the workspace; on chrB alone nobody has two
    names, pos, off, totals = reldist.point_arrays(annotations, ["chrB"])
    assert names == [] and len(pos) == 0 and off.tolist() == [0]
    names, pos, off, totals = reldist.point_arrays(annotations, ["chrC", "chrD"])
    assert names == ["three"] and off.tolist() == [0, 3, 3] and totals == [3]
    with pytest.raises(ValueError, match="annotation-point"):
        reldist.point_arrays(annotations, ["chrA"], "centre")
    # through the isochores the pieces of a contig are put together again, as fromIsochores does it: adjacent intervals unite
    _, iso, _, _ = inputs(tmp_path, ["--isochores=%s" % os.path.join(CLI, "isochores.bed")])
    names, pos, off, totals = reldist.point_arrays(iso, ["chrB", "chrA", "chrC"])
    assert names == ["one", "three"] and pos.tolist() == [15001, 20100, 30000, 20010, 20035] and off.tolist() == [0, 1, 3, 3, 3, 3, 5]


def test_points_of():
    from gat_amd import reldist
    a = np.array([(10, 20), (20, 21), (30, 33), (40, 42)], dtype=[("start", "<u4"), ("end", "<u4")])
    assert reldist.points_of(a).tolist() == [15, 20, 31, 41] and reldist.points_of(a, "start").tolist() == [10, 20, 30, 40]
    assert reldist.points_of(a, "end").tolist() == [19, 20, 32, 41] and reldist.points_of(a[:0]).tolist() == []
    for bad in ([(10, 20), (15, 30)], [(10, 10)], [(30, 40), (10, 20)]):
        with pytest.raises(AssertionError):
            reldist.points_of(np.array(bad, dtype=a.dtype))


def hand_table():
    from gat_amd import reldist
    S, B = 4, 2
    v = np.zeros((S, 2, B + 3), dtype=np.int64)              # two annotations, two bins: v_0, v_1, area, inside, outside
    v[:, 0] = [[1, 0, 250000, 1, 3], [0, 0, 0, 0, 4], [2, 2, 0, 4, 0], [0, 3, 250000, 3, 1]]
    v[:, 1] = [[0, 0, 0, 0, 4]] * 4
    obs = np.array([[2, 0, 250000, 2, 2], [0, 0, 0, 0, 4]], dtype=np.int64)
    return reldist.rows("trk", ["A", "B"], [5, 2], B, obs, M.words(v, obs), S), reldist


def test_rows_and_table():
    res, reldist = hand_table()
    # every bin of every annotation is a row, zeros included, then area, inside, outside
    assert [(x.annotation, x.bin, x.reldist_start, x.reldist_end, x.observed, x.samples_with_hit, x.points) for x in res] == [
        ("A", 0, 0.0, 0.25, 2, 2, 5), ("A", 1, 0.25, 0.5, 0, 2, 5), ("A", "area", 0.0, 0.5, 0.25, 2, 5), ("A", "inside", 0.0, 0.5, 2, 3, 5),
        ("A", "outside", 0.0, 0.5, 2, 3, 5), ("B", 0, 0.0, 0.25, 0, 0, 2), ("B", 1, 0.25, 0.5, 0, 0, 2), ("B", "area", 0.0, 0.5, 0.0, 0, 2),
        ("B", "inside", 0.0, 0.5, 0, 0, 2), ("B", "outside", 0.0, 0.5, 4, 4, 2)]
    b0, area, empty = res[0], res[2], res[5]
    assert (empty.expected, empty.stddev, empty.fold, empty.pvalue) == (0.0, 0.0, 1.0, 1.0)
    assert (b0.expected, b0.pvalue) == (0.75, 0.25) and b0.fold == 3.0 / 1.75
    # the area row: the statistics of the integers (parts per million), printed as fractions of 1
    assert area.words == (2, 500000, 2 * 250000 ** 2, 2, 2) and (area.observed, area.expected) == (0.25, 0.125) and area.stddev == 0.125
    assert area.fold == 250001.0 / 125001.0 and area.pvalue == 0.5
    reldist.set_qvalues(res, "none")
    assert str(b0) == "trk\tA\t0\t0\t0.25\t2\t0.7500\t0.8292\t1.7143\t0.7776\t2.5000e-01\t2.5000e-01\t2\t5"
    assert str(area) == "trk\tA\tarea\t0\t0.5\t0.250000\t0.1250\t0.1250\t2.0000\t1.0000\t5.0000e-01\t5.0000e-01\t2\t5"
    assert str(res[9]).split("\t")[2:6] == ["outside", "0", "0.5", "4"]
    fine = reldist.rows("trk", ["A"], [2], 1024, np.zeros((1, 1027), dtype=np.int64), np.zeros((1, 1027, 5), dtype=np.int64), 1)
    assert str(fine[1]).split("\t")[3:5] == ["0.000488281", "0.000976562"] and str(fine[1023]).split("\t")[3:5] == ["0.499512", "0.5"]
    sink = io.StringIO()
    reldist.write_results(sink, res, "track")
    lines = sink.getvalue().splitlines()
    assert lines[0].split("\t") == list(reldist.HEADER) and len(reldist.HEADER) == 14 and len(lines) == 11
    order = ["0", "1", "area", "inside", "outside"]
    assert [l.split("\t")[1:3] for l in lines[1:]] == [[t, b] for t in "AB" for b in order]
    more, _ = hand_table()
    for x in more:
        x.track = "a-first"
    sink = io.StringIO()
    reldist.write_results(sink, res + more, "annotation")
    assert [l.split("\t")[:3] for l in sink.getvalue().splitlines()[1:]] == [[k, t, b] for t in "AB" for k in ("a-first", "trk") for b in order]
    sink = io.StringIO()
    reldist.write_results(sink, res, "pvalue")
    keyed = [float(l.split("\t")[10]) for l in sink.getvalue().splitlines()[1:]]
    assert keyed == sorted(keyed) and keyed[0] == 0.25
    with pytest.raises(ValueError, match="unknown sort order"):
        reldist.write_results(io.StringIO(), res, "nothing")
    with pytest.raises(AssertionError):
        reldist.rows("trk", ["A"], [2], 3, np.zeros((1, 5), dtype=np.int64), np.zeros((1, 5, 5), dtype=np.int64), 1)


def test_qvalue_families():
    """per segment track: the bin rows are one family, the area rows another; inside and outside keep 1"""
    from gat_amd import reldist, stats
    res, _ = hand_table()
    more, _ = hand_table()
    for x in more[:5]:
        x.track = "other"
    both = res + more[:5]
    for x in both:
        x.qvalue = 0.5
    reldist.set_qvalues(both, "BH")
    for family in (res, more[:5]):
        bins, areas = [x for x in family if x.is_bin], [x for x in family if x.bin == "area"]
        assert len(bins) == 2 * len(areas) and len(areas) in (1, 2)
        assert [x.qvalue for x in bins] == stats.adjustPValues([x.pvalue for x in bins], method="BH").tolist()
        assert [x.qvalue for x in areas] == stats.adjustPValues([x.pvalue for x in areas], method="BH").tolist()
        assert all(x.qvalue == 1.0 for x in family if x.bin in ("inside", "outside"))
    # p-values set by hand: one family of all ten rows would give the first bin 0.01 * 10 / 5 and the first area 0.02 * 10 / 6
    for x, pv in zip(res, (0.01, 0.5, 0.02, 0.001, 0.001, 0.6, 0.7, 0.9, 0.001, 0.001)):
        x.pvalue = pv
    reldist.set_qvalues(res, "BH")
    assert [x.qvalue for x in res] == [0.04, 0.7, 0.04, 1.0, 1.0, 0.7, 0.7, 0.9, 1.0, 1.0]
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(ValueError, match="qvalue-method"):
            reldist.set_qvalues(res, bad)


def test_parser_and_what_is_refused():
    import gat_amd
    from gat_amd import reldist
    mod = script()
    opts, args = mod.buildParser().parse_args([])
    assert args == [] and opts.bins == 50 == reldist.BINS
    assert (opts.annotation_point, opts.qvalue_method, opts.sampler) == ("midpoint", "BH", "annotator")
    opts, _ = mod.buildParser().parse_args(["--segments=s.bed", "--annotations=a.bed", "--annotations=b.bed", "--workspace=w.bed",
                                            "--isochores=i.bed", "--annotation-point=end", "--bins=1024", "-q", "holm", "--order=track",
                                            "--num-samples=20", "--random-seed=4", "--pseudo-count=0.5"])
    assert (opts.segment_files, opts.annotation_files, opts.workspace_files) == (["s.bed"], ["a.bed", "b.bed"], ["w.bed"])
    assert (opts.annotation_point, opts.bins, opts.qvalue_method, opts.output_order, opts.num_samples, opts.random_seed,
            opts.pseudo_count) == ("end", 1024, "holm", "track", 20, 4, 0.5)
    for name in gat_amd.TOOL_SAMPLERS:
        assert mod.buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in reldist.QVALUE_METHODS:
        assert mod.buildParser().parse_args(["--qvalue-method=%s" % name])[0].qvalue_method == name
    for bad in (["--qvalue-method=storey"], ["--qvalue-method=minp"], ["--annotation-point=centre"], ["--counter=x"], ["--descriptions=d.tsv"],
                ["--bins=many"]):
        with pytest.raises(SystemExit):
            mod.buildParser().parse_args(bad)
    for argv, what in ((["--conditional=cooccurance"], "conditional"), (["--annotations-to-points=midpoint"], "annotations-to-points"),
                       (["--reference-stream"], "reference-stream")):
        with pytest.raises(NotImplementedError, match=what):
            mod.main(["gat-reldist.py"] + argv)
    for argv in (["--bins=0"], ["--bins=-3"], ["--bins=1025"]):
        with pytest.raises(ValueError, match="--bins"):
            mod.main(["gat-reldist.py"] + argv)
    assert reldist.check_bins(1) == 1 and reldist.check_bins(1024) == 1024
    with pytest.raises(NotImplementedError, match="run on the GPU path"):
        reldist.track_reldist("t", None, None, None, object(), 10)


def test_run_refuses_before_the_device(tmp_path, monkeypatch):
    from gat_amd import reldist
    segments, annotations, workspace, opts = inputs(tmp_path)
    monkeypatch.setattr(reldist, "get_context", lambda: pytest.fail("the device was asked"))
    sampler = reldist.make_sampler(opts)
    for kw, what in ((dict(n_bins=0), "--bins"), (dict(n_bins=1025), "--bins"), (dict(annotation_point="centre"), "annotation-point")):
        with pytest.raises(ValueError, match=what):
            reldist.run(segments, annotations, workspace, sampler, 10, random_seed=1, **kw)
    with pytest.raises(ValueError, match="num_samples"):
        reldist.run(segments, annotations, workspace, sampler, 0, random_seed=1)
    with pytest.raises(ValueError, match="qvalue-method"):
        reldist.run(segments, annotations, workspace, sampler, 10, qvalue_method="storey")

    class Few(object):          # an annotation collection without two points on any contig: no row, and the device is not asked
        tracks = ["two"]

        def __getitem__(self, name):
            return annotations[name]
    assert reldist.run(segments, Few(), workspace, sampler, 10, random_seed=1) == []
