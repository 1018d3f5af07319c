"""CPU: gat-signal's host side -- bedGraph files, the quantisation, the tracks' names, the counters' values from the four
words, the rows made from a hand-made [samples][tracks][4] array, the command line's choices and defaults, what it refuses."""
import gzip
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def script():
    spec = importlib.util.spec_from_file_location("gat_signal_cli", os.path.join(ROOT, "scripts", "gat-signal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BEDGRAPH = """track type=bedGraph name="x"
browser position chr1:1-100
# a comment
chr1\t10\t20\t0.5
chr2\t0\t5\t-1.25
chr1\t0\t10\t2
chr1\t30\t30\t9

chr1\t20\t25\t0
"""


def test_bedgraph_header_lines_order_and_zero_length_pieces(tmp_path):
    from gat_amd import signals
    path = tmp_path / "cons.bedGraph"
    path.write_text(BEDGRAPH)
    t = signals.read_bedgraph(str(path), 1000)
    assert t.name == "cons" and list(t.pieces) == ["chr1", "chr2"]
    p, q = t.pieces["chr1"]
    assert p["start"].tolist() == [0, 10, 20] and p["end"].tolist() == [10, 20, 25]          # sorted; the zero-length piece dropped
    assert q.dtype == np.int32 and q.tolist() == [2000, 500, 0]
    assert t.pieces["chr2"][0].tolist() == [(0, 5)] and t.pieces["chr2"][1].tolist() == [-1250]
    gz = tmp_path / "cons.copy.bedGraph.gz"
    with gzip.open(str(gz), "wt") as f:
        f.write(BEDGRAPH)
    g = signals.read_bedgraph(str(gz), 1000)
    assert g.name == "cons.copy" and g.pieces["chr1"][1].tolist() == [2000, 500, 0]
    assert np.array_equal(g.pieces["chr1"][0], p)


def test_bedgraph_errors_name_the_file_and_the_contig(tmp_path):
    from gat_amd import signals
    path = tmp_path / "bad.bg"
    path.write_text("chr1\t0\t10\t1\nchr7\t5\t9\t1\nchr7\t8\t12\t1\n")
    with pytest.raises(ValueError, match=r"bad\.bg: overlapping pieces on contig chr7"):
        signals.read_bedgraph(str(path))
    path.write_text("chr1\t0\t10\n")
    with pytest.raises(ValueError, match="four columns"):
        signals.read_bedgraph(str(path))
    path.write_text("chr1\t0\t10\tnan\n")
    with pytest.raises(ValueError, match=r"bad\.bg: contig chr1: .*not finite"):
        signals.read_bedgraph(str(path))
    path.write_text("chr1\t0\t10\t3000000\n")
    with pytest.raises(ValueError, match="beyond 2\\^31 - 1"):
        signals.read_bedgraph(str(path), 1000)
    assert signals.read_bedgraph(str(path), 1).pieces["chr1"][1].tolist() == [3000000]
    path.write_text("chr1\t0\t10\t1\nchr1\t10\t12\t1\n")                      # adjacent pieces are no overlap
    assert len(signals.read_bedgraph(str(path)).pieces["chr1"][0]) == 2


def test_quantisation_rounds_half_to_even_and_checks_the_range():
    from gat_amd import signals
    q = signals.quantise([0.5, 1.5, 2.5, -0.5, -1.5, 0.0004, 0.0006, -0.0016], 1)
    assert q.dtype == np.int32 and q.tolist() == [0, 2, 2, 0, -2, 0, 0, 0]
    assert signals.quantise([0.0005, 0.0015, 0.0025, -0.0035, 1.0], 1000).tolist()[4] == 1000
    assert signals.quantise([0.5, 1.5, 2.5, 3.5, -2.5], 1).tolist() == [0, 2, 2, 4, -2]
    top = 2 ** 31 - 1
    assert signals.quantise([top, -top], 1).tolist() == [top, -top]
    for bad in ([2 ** 31], [-2 ** 31], [float(top) + 0.5], [2147483.648]):
        with pytest.raises(ValueError, match="2\\^31 - 1"):
            signals.quantise(bad, 1000 if bad == [2147483.648] else 1)
    for bad in ([float("nan")], [float("inf")], [1.0, -float("inf")]):
        with pytest.raises(ValueError, match="not finite"):
            signals.quantise(bad, 1000)
    assert signals.quantise([], 1000).dtype == np.int32 and len(signals.quantise([], 1000)) == 0


def test_track_names_and_collisions(tmp_path):
    from gat_amd import signals
    assert signals.track_name("/a/b/phastcons.bedGraph.gz") == "phastcons"
    assert signals.track_name("gc.5kb.bg") == "gc.5kb" and signals.track_name("plain") == "plain" and signals.track_name("x.gz") == "x"
    for sub, name in (("one", "sig.bedGraph"), ("two", "sig.bg.gz")):
        os.makedirs(str(tmp_path / sub))
        opener = gzip.open if name.endswith(".gz") else open
        with opener(str(tmp_path / sub / name), "wt") as f:
            f.write("chr1\t0\t10\t1\n")
    a, b = str(tmp_path / "one" / "sig.bedGraph"), str(tmp_path / "two" / "sig.bg.gz")
    with pytest.raises(ValueError, match="both track 'sig'"):
        signals.read_tracks([a, b])
    assert [t.name for t in signals.read_tracks([a])] == ["sig"]


def test_piece_lists_are_track_major_with_empty_lists_for_missing_contigs(tmp_path):
    from gat_amd import signals
    (tmp_path / "a.bg").write_text("c2\t5\t9\t1\nc1\t0\t4\t2\nc9\t0\t4\t7\n")
    (tmp_path / "b.bg").write_text("c2\t1\t2\t-3\n")
    tracks = signals.read_tracks([str(tmp_path / "a.bg"), str(tmp_path / "b.bg")], 1)
    segs, vals, off = signals.piece_lists(tracks, ["c1", "c2", "c3"])                       # (c9 is not the problem's: ignored)
    assert off.tolist() == [0, 1, 2, 2, 2, 3, 3] and off.dtype == np.int64
    assert segs["start"].tolist() == [0, 5, 1] and vals.tolist() == [2, 1, -3] and vals.dtype == np.int32
    segs, vals, off = signals.piece_lists([], ["c1"])
    assert len(segs) == 0 and len(vals) == 0 and off.tolist() == [0]


def test_values_of_the_four_words():
    from gat_amd import signals
    words = np.array([[[4, 10, 3, 25000], [2, 0, 0, 0]], [[3, 4, 1, -2 ** 40], [1, 1, 1, 1]]], dtype=np.int64)
    v = signals.values(words, "signal-mean", 1000)
    assert v.dtype == np.float64 and v.tolist() == [[2.5, 0.0], [-2 ** 40 / 4 / 1000.0, 0.001]]       # (covered == 0: 0.0, not a division)
    assert signals.values(words, "signal-sum", 1000).tolist() == [[25.0, 0.0], [-2 ** 40 / 1000.0, 0.001]]
    assert signals.values(words, "signal-covered").tolist() == [[10.0, 0.0], [4.0, 1.0]]
    assert signals.values(words, "signal-hit").tolist() == [[3.0, 0.0], [1.0, 1.0]]
    for name in signals.COUNTER_NAMES:
        assert signals.values(words, name).dtype == np.float64 and signals.values(np.zeros((0, 2, 4), dtype=np.int64), name).shape == (0, 2)
    with pytest.raises(ValueError):
        signals.values(words, "nucleotide-overlap")
    assert signals.observed_format(["signal-covered", "signal-hit"]) == "%i"
    assert signals.observed_format(["signal-hit", "signal-mean"]) == signals.observed_format(["signal-sum"]) == "%6.4f"
    assert signals.WORDS == ("n", "covered", "hit", "sum")


def test_rows_from_hand_made_words():
    from gat_amd import engine, signals
    sample = np.array([[[2, 10, 1, 10000], [2, 0, 0, 0]],
                       [[2, 20, 2, 40000], [2, 5, 1, -5000]],
                       [[2, 10, 1, 30000], [2, 5, 1, 5000]],
                       [[2, 40, 2, 40000], [2, 0, 0, 0]]], dtype=np.int64)
    observed = np.array([[2, 10, 2, 50000], [2, 4, 1, -8000]], dtype=np.int64)
    a, b = signals.rows("merged", ["cons", "gc"], "signal-mean", observed, sample, 1000)
    assert type(a) is engine.AnnotatorResult and (a.track, a.annotation, a.counter) == ("merged", "cons", "signal-mean")
    assert a.observed == 5.0 and a.samples.tolist() == [1.0, 2.0, 3.0, 1.0] and a.expected == 1.75
    assert a.fold == 5.0 / 1.75                                              # the pseudo count is 0 here
    assert b.observed == -2.0 and b.samples.tolist() == [0.0, -1.0, 1.0, 0.0]
    want = engine.AnnotatorResult("merged", "cons", "signal-mean", 5.0, [1.0, 2.0, 3.0, 1.0], pseudo_count=0.0)
    assert str(a) == str(want)
    hit = signals.rows("merged", ["cons", "gc"], "signal-hit", observed, sample, 1000, pseudo_count=1.0)
    assert hit[0].observed == 2.0 and hit[0].samples.tolist() == [1.0, 2.0, 1.0, 2.0] and hit[0].fold == 3.0 / 2.5


def test_parser_defaults_and_options():
    import gat_amd
    from gat_amd import signals
    parser = script().buildParser()
    opts, args = parser.parse_args([])
    assert args == [] and opts.counters == [] and opts.signal_files == [] and opts.signal_scale == 1000 and opts.pseudo_count == 0
    assert opts.sampler == "annotator" and opts.num_samples == 1000 and opts.qvalue_method == "BH" and opts.output_order == "fold"
    assert not parser.has_option("--annotations") and not parser.has_option("-a") and parser.has_option("--pseudo-count")
    assert gat_amd.buildParser().parse_args([])[0].pseudo_count == 1.0 and gat_amd.buildParser().has_option("--annotations")
    assert signals.COUNTER_NAMES == ("signal-mean", "signal-sum", "signal-covered", "signal-hit") and signals.SCALE == 1000
    opts, _ = script().buildParser().parse_args(
        ["--segments=s.bed", "--signal=a.bedGraph", "--signal=b.bg.gz", "--workspace=w.bed", "--isochores=i.bed", "--with-segment-tracks",
         "--sampler=brute-force", "--num-samples=20", "--random-seed=4", "--signal-scale=10", "--pseudo-count=0.5", "--qvalue-method=minp",
         "--counter=signal-hit", "-c", "signal-sum", "--stdout=o.tsv", "--verbose=0"])
    assert opts.segment_files == ["s.bed"] and opts.signal_files == ["a.bedGraph", "b.bg.gz"] and opts.workspace_files == ["w.bed"]
    assert (opts.num_samples, opts.random_seed, opts.signal_scale, opts.pseudo_count, opts.qvalue_method) == (20, 4, 10.0, 0.5, "minp")
    assert opts.counters == ["signal-hit", "signal-sum"] and opts.sampler == "brute-force"
    for name in gat_amd.CLI_SAMPLERS:
        assert script().buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in ("efdr", "minp", "storey", "none"):
        assert script().buildParser().parse_args(["--qvalue-method=%s" % name])[0].qvalue_method == name


def test_counter_choices_are_the_scripts_own(capsys):
    import gat_amd
    with pytest.raises(SystemExit):
        script().buildParser().parse_args(["--counter=nucleotide-overlap"])
    assert "invalid choice" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        script().buildParser().parse_args(["--annotations=a.bed"])
    capsys.readouterr()
    with pytest.raises(SystemExit):                       # gat-run.py's parser is as it was
        gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS).parse_args(["--counter=signal-mean"])
    assert not gat_amd.buildParser().has_option("--signal")


@pytest.mark.parametrize("extra,error", [(["--conditional=cooccurance"], NotImplementedError), (["--reference-stream"], NotImplementedError),
                                         (["--annotations-to-points=midpoint"], NotImplementedError),
                                         (["--truncate-workspace-to-annotations"], NotImplementedError),
                                         (["--signal-scale=0"], ValueError), (["--signal-scale=nan"], ValueError), (["no-signal"], ValueError)])
def test_what_is_refused(extra, error, tmp_path):
    sig = tmp_path / "sig.bedGraph"
    sig.write_text("chr1\t0\t10\t1\n")
    argv = ["gat-signal.py", "--segments=%s" % os.path.join(CLI, "segments.bed"), "--workspace=%s" % os.path.join(CLI, "workspace.bed"),
            "--stdout=%s" % (tmp_path / "out.tsv")]
    if extra != ["no-signal"]:
        argv += ["--signal=%s" % sig] + extra
    with pytest.raises(error):
        script().main(argv)
    assert not os.path.exists(tmp_path / "out.tsv")             # (refused before anything is read or opened)


def test_module_imports_without_a_device():
    from gat_amd import signals
    assert callable(signals.run)
    sampler = signals.make_sampler(script().buildParser().parse_args([])[0])
    with pytest.raises(ValueError):
        signals.track_signal("t", None, [], None, sampler, ["overlap"], 5)
    with pytest.raises(NotImplementedError):
        signals.track_signal("t", None, [], None, object(), ["signal-mean"], 5)
