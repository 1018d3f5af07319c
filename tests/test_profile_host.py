"""CPU: gat-profile's host side -- the anchors read from BED files (track names as io.readFromBed has them, the strand column,
the three anchor points, duplicates, --ignore-strand, --annotations-label), what is refused, and the table: every bin a row,
the offsets, the orders."""
import importlib.util
import io
import os

import numpy as np
import pytest

import profile_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")

BED = """\
# a comment
chr1\t100\t200\tgeneA\t0\t+
chr1\t300\t400\tgeneB\t0\t-
chr2\t50\t51\tgeneA\t0\t-
chr1\t100\t250\tgeneA\t0\t+
chr1\t100\t200\tgeneA\t0\t-
chr1\t10\t20\tgeneA\t0\t.
chr2\t7\t9\tgeneB
chr1\t10\t15
"""
TRACKS = """\
track name="tss" description="x"
chr1\t100\t200\tignored\t0\t-
chr1\t90\t95\tignored\t0\t+
track name=ends
chrX\t5\t6\tn\t0\t-
"""


def script():
    spec = importlib.util.spec_from_file_location("gat_profile_cli", os.path.join(ROOT, "scripts", "gat-profile.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def beds(tmp_path):
    a, b = tmp_path / "anchors.bed", tmp_path / "tracks.bed"
    a.write_text(BED)
    b.write_text(TRACKS)
    return str(a), str(b)


def as_lists(anchors):
    return {t: {c: list(zip(p.tolist(), m.tolist())) for c, (p, m) in per.items()} for t, per in anchors.items()}


def test_read_anchors(beds, monkeypatch):
    from gat_amd import io as IO, profile
    monkeypatch.setenv("GAT_BED_LINE_READER", "1")
    a, b = beds
    got = profile.read_anchors([a, b])
    ref = IO.readFromBed([a, b])
    assert list(got) == list(ref) == ["geneA", "geneB", "anchors.bed", "tss", "ends"]
    for t in got:
        assert list(got[t]) == list(ref[t].keys())
        for p, m in got[t].values():
            assert p.dtype == np.uint32 and m.dtype == np.uint8
    # five-prime: plus -> start; minus -> end - 1 (end == start + 1: the start); '.' and a missing column are plus; the same
    # (position, strand) of two transcripts once; plus before minus at one position
    assert as_lists(got) == {"geneA": {"chr1": [(10, 0), (100, 0), (199, 1)], "chr2": [(50, 1)]},
                             "geneB": {"chr1": [(399, 1)], "chr2": [(7, 0)]},
                             "anchors.bed": {"chr1": [(10, 0)]},
                             "tss": {"chr1": [(90, 0), (199, 1)]}, "ends": {"chrX": [(5, 1)]}}
    assert as_lists(profile.read_anchors(a, "three-prime")) == {
        "geneA": {"chr1": [(19, 0), (100, 1), (199, 0), (249, 0)], "chr2": [(50, 1)]},
        "geneB": {"chr1": [(300, 1)], "chr2": [(8, 0)]}, "anchors.bed": {"chr1": [(14, 0)]}}
    assert as_lists(profile.read_anchors(a, "midpoint")) == {
        "geneA": {"chr1": [(15, 0), (150, 0), (150, 1), (175, 0)], "chr2": [(50, 1)]},
        "geneB": {"chr1": [(350, 1)], "chr2": [(8, 0)]}, "anchors.bed": {"chr1": [(12, 0)]}}
    # --ignore-strand: every anchor plus, so the minus intervals anchor at their start and collapse with the plus ones
    assert as_lists(profile.read_anchors(a, "five-prime", ignore_strand=True)) == {
        "geneA": {"chr1": [(10, 0), (100, 0)], "chr2": [(50, 0)]}, "geneB": {"chr1": [(300, 0)], "chr2": [(7, 0)]},
        "anchors.bed": {"chr1": [(10, 0)]}}
    # --annotations-label: one track, named as the annotation collection names it
    pooled = profile.read_anchors([a, b], label="anything")
    assert list(pooled) == list(IO.readFromBed([a, b], allow_multiple=True, ignore_tracks=True)) == ["merged"]
    assert as_lists(pooled)["merged"] == {"chr1": [(10, 0), (90, 0), (100, 0), (199, 1), (399, 1)], "chr2": [(7, 0), (50, 1)], "chrX": [(5, 1)]}
    with pytest.raises(ValueError, match="anchor-point"):
        profile.read_anchors(a, "centre")


def test_anchor_position():
    from gat_amd.profile import anchor_position as f
    assert [f(100, 200, False, p) for p in ("five-prime", "three-prime", "midpoint")] == [100, 199, 150]
    assert [f(100, 200, True, p) for p in ("five-prime", "three-prime", "midpoint")] == [199, 100, 150]
    assert [f(7, 8, m, p) for m in (False, True) for p in ("five-prime", "three-prime", "midpoint")] == [7] * 6
    assert f(7, 7, True, "five-prime") == 7 and f(7, 10, True, "midpoint") == 8 and f(7, 9, False, "midpoint") == 8


def test_anchor_arrays(beds):
    """tracks without an anchor on the problem's contigs are left out, anchors on other contigs dropped; the offsets are
    track-major over the problem's contigs in the problem's order"""
    from gat_amd import profile
    anchors = profile.read_anchors(list(beds))
    names, pos, minus, off, totals = profile.anchor_arrays(anchors, ["chr2", "chr1"])
    assert names == ["geneA", "geneB", "anchors.bed", "tss"] and totals == [4, 2, 1, 2]
    assert off.tolist() == [0, 1, 4, 5, 6, 6, 7, 7, 9] and pos.dtype == np.uint32 and minus.dtype == np.uint8
    assert pos.tolist() == [50, 10, 100, 199, 7, 399, 10, 90, 199] and minus.tolist() == [1, 0, 0, 1, 0, 1, 0, 0, 1]
    names, pos, minus, off, totals = profile.anchor_arrays(anchors, ["chr9"])
    assert names == [] and len(pos) == 0 and off.tolist() == [0]


def hand_table():
    from gat_amd import profile
    S = 4
    v = np.zeros((S, 2, 4), dtype=np.int64)                  # two anchor tracks, w = 10, H = 2
    v[:, 0, 1] = [0, 3, 3, 10]
    v[:, 1, 3] = [1, 0, 0, 0]
    v[:, 1, 0] = [2, 2, 2, 2]
    obs = np.zeros((2, 4), dtype=np.int64)
    obs[0, 1], obs[0, 2], obs[1, 0] = 3, 7, 2
    return profile.rows("trk", ["A", "B"], [5, 1], 10, 2, obs, M.words(v, obs), S), profile


def test_rows_and_table():
    res, profile = hand_table()
    # every bin of every track is a row, zeros included
    assert [(x.annotation, x.bin, x.offset_start, x.offset_end, x.observed, x.samples_with_overlap, x.anchors) for x in res] == [
        ("A", 0, -20, -10, 0, 0, 5), ("A", 1, -10, 0, 3, 3, 5), ("A", 2, 0, 10, 7, 0, 5), ("A", 3, 10, 20, 0, 0, 5),
        ("B", 0, -20, -10, 2, 4, 1), ("B", 1, -10, 0, 0, 0, 1), ("B", 2, 0, 10, 0, 0, 1), ("B", 3, 10, 20, 0, 1, 1)]
    empty, a = res[0], res[1]
    assert (empty.expected, empty.stddev, empty.fold, empty.pvalue) == (0.0, 0.0, 1.0, 1.0)
    assert (a.expected, a.pvalue) == (4.0, 0.75) and a.fold == 4.0 / 5.0
    profile.set_qvalues(res, "none")
    assert str(a) == "trk\tA\t1\t-10\t0\t3\t4.0000\t3.6742\t0.8000\t-0.3219\t7.5000e-01\t7.5000e-01\t3\t5"
    sink = io.StringIO()
    profile.write_results(sink, res, "track")
    lines = sink.getvalue().splitlines()
    assert lines[0].split("\t") == list(profile.HEADER) and len(profile.HEADER) == 14 and len(lines) == 9
    assert [l.split("\t")[1:3] for l in lines[1:]] == [[t, str(b)] for t in "AB" for b in range(4)]
    more, _ = hand_table()
    for x in more:
        x.track = "a-first"
    sink = io.StringIO()
    profile.write_results(sink, res + more, "annotation")
    assert [l.split("\t")[:3] for l in sink.getvalue().splitlines()[1:]] == [[k, t, str(b)] for t in "AB" for k in ("a-first", "trk") for b in range(4)]
    sink = io.StringIO()
    profile.write_results(sink, res, "pvalue")                # ties go by bin: the sort is stable over (track, annotation, bin)
    keyed = [(float(l.split("\t")[10]), l.split("\t")[1], int(l.split("\t")[2])) for l in sink.getvalue().splitlines()[1:]]
    assert keyed == sorted(keyed) and keyed[0][0] == 0.25
    sink = io.StringIO()
    profile.write_results(sink, res, "observed")
    assert [int(l.split("\t")[5]) for l in sink.getvalue().splitlines()[1:]] == [0, 0, 0, 0, 0, 2, 3, 7]
    with pytest.raises(ValueError, match="unknown sort order"):
        profile.write_results(io.StringIO(), res, "nothing")


def test_qvalues_per_track():
    from gat_amd import profile, stats
    res, _ = hand_table()
    more, _ = hand_table()
    for x in more[:3]:
        x.track = "other"
    profile.set_qvalues(res + more[:3], "BH")
    assert [x.qvalue for x in res] == stats.adjustPValues([x.pvalue for x in res], method="BH").tolist()
    assert [x.qvalue for x in more[:3]] == stats.adjustPValues([x.pvalue for x in more[:3]], method="BH").tolist()
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(ValueError, match="qvalue-method"):
            profile.set_qvalues(res, bad)


def test_parser_and_what_is_refused():
    import gat_amd
    from gat_amd import profile
    mod = script()
    opts, args = mod.buildParser().parse_args([])
    assert args == [] and (opts.bin_size, opts.half_bins) == (100, 50) == (profile.BIN_SIZE, profile.HALF_BINS)
    assert (opts.anchor_point, opts.ignore_strand, opts.profile_of, opts.qvalue_method, opts.sampler) == ("five-prime", False, "bases", "BH", "annotator")
    opts, _ = mod.buildParser().parse_args(["--segments=s.bed", "--anchors=a.bed", "--annotations=b.bed", "--workspace=w.bed",
                                            "--anchor-point=three-prime", "--ignore-strand", "--bin-size=10", "--half-bins=512",
                                            "--profile-of=midpoints", "-q", "holm", "--order=track", "--num-samples=20", "--random-seed=4"])
    assert (opts.segment_files, opts.annotation_files, opts.workspace_files) == (["s.bed"], ["a.bed", "b.bed"], ["w.bed"])
    assert (opts.anchor_point, opts.ignore_strand, opts.bin_size, opts.half_bins, opts.profile_of, opts.qvalue_method, opts.output_order,
            opts.num_samples, opts.random_seed) == ("three-prime", True, 10, 512, "midpoints", "holm", "track", 20, 4)
    for name in gat_amd.CLI_SAMPLERS:
        assert mod.buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in profile.QVALUE_METHODS:
        assert mod.buildParser().parse_args(["--qvalue-method=%s" % name])[0].qvalue_method == name
    for bad in (["--qvalue-method=storey"], ["--qvalue-method=minp"], ["--anchor-point=centre"], ["--profile-of=ends"], ["--counter=x"],
                ["--descriptions=d.tsv"]):
        with pytest.raises(SystemExit):
            mod.buildParser().parse_args(bad)
    for argv, what in ((["--conditional=cooccurance"], "conditional"), (["--annotations-to-points=midpoint"], "annotations-to-points"),
                       (["--reference-stream"], "reference-stream")):
        with pytest.raises(NotImplementedError, match=what):
            mod.main(["gat-profile.py"] + argv)
    for argv, what in ((["--bin-size=0"], "bin-size"), (["--bin-size=%d" % (2 ** 31 + 1)], "bin-size"), (["--half-bins=0"], "half-bins"),
                       (["--half-bins=513"], "half-bins"), (["--half-bins=512", "--bin-size=%d" % (2 ** 22 + 1)], "more than 2\\^31")):
        with pytest.raises(ValueError, match=what):
            mod.main(["gat-profile.py"] + argv)
    assert profile.check_geometry(2 ** 22, 512, "midpoints") == (2 ** 22, 512, 1) and profile.check_geometry(2 ** 31, 1) == (2 ** 31, 1, 0)
    with pytest.raises(NotImplementedError, match="run on the GPU path"):
        profile.track_profile("t", None, {}, None, object(), 10)


def test_run_refuses_before_the_device(monkeypatch):
    from gat_amd import profile
    mod = script()
    opts, _ = mod.buildParser().parse_args(["--segments=%s" % os.path.join(CLI, "segments.bed"),
                                            "--anchors=%s" % os.path.join(CLI, "annotations.bed"),
                                            "--workspace=%s" % os.path.join(CLI, "workspace.bed")])
    segments, annotations, workspace = profile.build_inputs(opts)
    monkeypatch.setattr(profile, "get_context", lambda: pytest.fail("the device was asked"))
    sampler = profile.make_sampler(opts)
    for kw, what in ((dict(bin_size=0), "bin-size"), (dict(half_bins=600), "half-bins"), (dict(profile_of="ends"), "profile-of")):
        with pytest.raises(ValueError, match=what):
            profile.run(segments, {}, workspace, sampler, 10, random_seed=1, **kw)
    with pytest.raises(ValueError, match="num_samples"):
        profile.run(segments, {}, workspace, sampler, 0, random_seed=1)
    with pytest.raises(ValueError, match="qvalue-method"):
        profile.run(segments, {}, workspace, sampler, 10, qvalue_method="storey")
    # anchors on contigs the problem lacks: no track is left, no row, and the device is not asked
    nowhere = {"far": {"no-such-contig": (np.array([5], dtype=np.uint32), np.array([0], dtype=np.uint8))}}
    assert profile.run(segments, nowhere, workspace, sampler, 10, random_seed=1) == []
