"""CPU: gat-distance's host side -- the command line's choices and defaults, what it refuses, the counters' values from the
four words, the rows made from a hand-made [samples][tracks][4] array."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def script():
    spec = importlib.util.spec_from_file_location("gat_distance_cli", os.path.join(ROOT, "scripts", "gat-distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parser_defaults_and_options():
    import gat_amd
    from gat_amd import distance
    opts, args = script().buildParser().parse_args([])
    assert args == [] and opts.counters == [] and opts.max_distance == 1000 and opts.sampler == "annotator"
    assert opts.num_samples == 1000 and opts.ignore_segment_tracks is True and opts.output_order == "fold" and opts.qvalue_method == "BH"
    assert distance.COUNTER_NAMES == ("segment-distance", "segment-nearby", "annotation-distance", "annotation-nearby")
    assert sorted(distance.COUNTERS) == sorted(distance.COUNTER_NAMES) and distance.MAX_DISTANCE == 1000
    opts, _ = script().buildParser().parse_args(
        ["--segments=s.bed", "--annotations=a.bed", "--workspace=w.bed", "--isochores=i.bed", "--with-segment-tracks",
         "--sampler=brute-force", "--num-samples=20", "--random-seed=4", "--max-distance=77", "--order=pvalue", "--qvalue-method=storey",
         "--descriptions=d.tsv", "--counter=annotation-nearby", "-c", "segment-distance", "--stdout=o.tsv", "--verbose=0"])
    assert opts.segment_files == ["s.bed"] and opts.annotation_files == ["a.bed"] and opts.workspace_files == ["w.bed"]
    assert opts.isochore_files == ["i.bed"] and opts.ignore_segment_tracks is False and opts.sampler == "brute-force"
    assert (opts.num_samples, opts.random_seed, opts.max_distance, opts.output_order, opts.qvalue_method) == (20, 4, 77, "pvalue", "storey")
    assert opts.input_filename_descriptions == "d.tsv" and opts.counters == ["annotation-nearby", "segment-distance"]
    for name in gat_amd.CLI_SAMPLERS:
        assert script().buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in distance.COUNTER_NAMES:
        assert script().buildParser().parse_args(["--counter=%s" % name])[0].counters == [name]


def test_counter_choices_are_the_scripts_own(capsys):
    import gat_amd
    with pytest.raises(SystemExit):
        script().buildParser().parse_args(["--counter=nucleotide-overlap"])
    assert "invalid choice" in capsys.readouterr().err
    with pytest.raises(SystemExit):                       # gat-run.py's parser is as it was
        gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS).parse_args(["--counter=segment-distance"])
    assert gat_amd.buildParser().parse_args(["--counter=nucleotide-overlap"])[0].counters == ["nucleotide-overlap"]
    assert not gat_amd.buildParser().has_option("--max-distance")


@pytest.mark.parametrize("extra", [["--conditional=cooccurance"], ["--conditional=segment-centered", "--conditional-expansion=2"],
                                   ["--annotations-to-points=midpoint"], ["--reference-stream"]])
def test_what_is_refused(extra, tmp_path):
    argv = ["gat-distance.py", "--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--stdout=%s" % (tmp_path / "out.tsv")]
    with pytest.raises(NotImplementedError):
        script().main(argv + extra)
    assert not os.path.exists(tmp_path / "out.tsv")             # (refused before anything is read or opened)


def test_module_imports_without_a_device():
    from gat_amd import distance
    assert callable(distance.run) and distance.WORDS == ("n", "sum", "near", "none")
    with pytest.raises(ValueError):
        distance.track_distances("t", None, None, None, distance.make_sampler(script().buildParser().parse_args([])[0]), ["overlap"], 5)
    with pytest.raises(NotImplementedError):
        distance.track_distances("t", None, None, None, object(), ["segment-distance"], 5)


def test_values_of_the_four_words():
    from gat_amd import distance
    words = np.array([[[4, 10, 3, 0], [0, 0, 0, 7]], [[3, 2 ** 40, 0, 1], [1, 1, 1, 0]]], dtype=np.int64)
    for name in ("segment-distance", "annotation-distance"):
        v = distance.values(words, name)
        assert v.dtype == np.float64 and v.tolist() == [[2.5, 0.0], [2 ** 40 / 3.0, 1.0]]          # (n == 0: 0.0, not a division)
    for name in ("segment-nearby", "annotation-nearby"):
        v = distance.values(words, name)
        assert v.dtype == np.float64 and v.tolist() == [[3.0, 0.0], [0.0, 1.0]]
    assert distance.values(np.zeros((0, 2, 4), dtype=np.int64), "segment-distance").shape == (0, 2)
    assert distance.observed_format(["segment-nearby", "annotation-nearby"]) == "%i"
    assert distance.observed_format(["segment-nearby", "annotation-distance"]) == "%6.4f"
    assert distance.COUNTERS["segment-distance"][0] == distance.COUNTERS["segment-nearby"][0] == 0
    assert distance.COUNTERS["annotation-distance"][0] == distance.COUNTERS["annotation-nearby"][0] == 1


def test_rows_from_hand_made_words():
    from gat_amd import distance, engine
    # five samples, two tracks
    sample = np.array([[[2, 10, 1, 0], [2, 40, 0, 0]],
                       [[2, 20, 2, 0], [2, 40, 0, 0]],
                       [[2, 30, 0, 0], [0, 0, 0, 2]],
                       [[2, 40, 1, 0], [2, 80, 2, 0]],
                       [[1, 50, 1, 1], [2, 40, 1, 0]]], dtype=np.int64)
    observed = np.array([[2, 4, 2, 0], [2, 100, 0, 0]], dtype=np.int64)
    rows = distance.rows("merged", ["near_tss", "far"], "segment-distance", observed, sample, pseudo_count=1.0)
    assert [type(r) for r in rows] == [engine.AnnotatorResult] * 2
    assert [(r.track, r.annotation, r.counter) for r in rows] == [("merged", "near_tss", "segment-distance"), ("merged", "far", "segment-distance")]
    a, b = rows
    assert a.observed == 2.0 and a.samples.tolist() == [5.0, 10.0, 15.0, 20.0, 50.0] and a.expected == 20.0
    assert a.fold == (2.0 + 1.0) / (20.0 + 1.0) and a.fold < 1                          # closer than expected
    assert a.pvalue == engine.getTwoSidedPValue(np.sort(a.samples), a.expected, a.observed) == 0.2
    assert b.observed == 50.0 and b.samples.tolist() == [20.0, 20.0, 0.0, 40.0, 20.0] and b.expected == 20.0 and b.fold > 1
    want = engine.AnnotatorResult("merged", "near_tss", "segment-distance", 2.0, [5.0, 10.0, 15.0, 20.0, 50.0])
    assert str(a) == str(want)
    near = distance.rows("merged", ["near_tss", "far"], "segment-nearby", observed, sample)
    assert near[0].observed == 2.0 and near[0].samples.tolist() == [1.0, 2.0, 0.0, 1.0, 1.0]
    assert near[1].observed == 0.0 and near[1].samples.tolist() == [0.0, 0.0, 0.0, 2.0, 1.0]


def test_contig_lists_are_entity_major_with_empty_lists_for_missing_contigs():
    from gat_amd import distance, intervals
    a, b = intervals.make([1, 5], [2, 9]), intervals.make([7], [8])
    data, off = distance.contig_lists([{"c1": a}, {"c2": b, "c1": b}], ["c1", "c2", "c3"])
    assert off.tolist() == [0, 2, 2, 2, 3, 4, 4] and off.dtype == np.int64
    assert data["start"].tolist() == [1, 5, 7, 7] and data.dtype == intervals.SEG
    data, off = distance.contig_lists([{}], ["c1"])
    assert len(data) == 0 and off.tolist() == [0, 0]
