"""CPU: the host side of --output-stats=segment_metrics / sample_metrics -- the options parse, the side files are opened
through -P / --force with the headers where the reference writes them, `all` opens neither, what cannot be measured is
refused before anything is sampled, and run()'s segment_metrics block writes the reference's file when the device's sums are
the model's."""
import importlib.util
import io
import json
import os

import numpy as np
import pytest

import metrics_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
GOLD = os.path.join(ROOT, "tests", "golden", "metrics", "cli")
HEADER = "track\tsection\tmetric\tnval\tmin\tmax\tmean\tmedian\tstddev\tsum\tq1\tq3\n"


def script():
    spec = importlib.util.spec_from_file_location("gat_run_cli_metrics", os.path.join(ROOT, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def base_argv(tmp_path, extra):
    extra = [x.replace("--isochores=", "--isochores=%s%s" % (CLI, os.sep)) for x in extra]
    return ["gat-run.py", "--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--stdout=%s" % (tmp_path / "table.tsv"),
            "--log=%s" % (tmp_path / "log")] + extra


def test_the_options_are_accepted():
    import gat_amd
    for parser in (gat_amd.buildParser(), gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS)):
        opts, _ = parser.parse_args(["--output-stats=sample_metrics", "--output-stats=segment_metrics", "--output-stats=all"])
        assert opts.output_stats == ["sample_metrics", "segment_metrics", "all"]
    assert gat_amd.buildParser().parse_args([])[0].output_stats == []


def test_unknown_section_is_still_refused(capsys):
    import gat_amd
    with pytest.raises(SystemExit):
        gat_amd.buildParser().parse_args(["--output-stats=sample_metric"])
    assert "invalid choice" in capsys.readouterr().err


@pytest.fixture()
def captured(monkeypatch):
    """gat_amd.fromSegments with run() replaced: what it was handed, after the inputs were prepared"""
    import gat_amd
    seen = {}

    def stub(segments, annotations, workspace, sampler, counters, workspace_generator, **kwargs):
        seen["outfiles"] = dict(kwargs["outfiles"])
        for f in seen["outfiles"].values():
            f.flush()
        return []

    monkeypatch.setattr(gat_amd, "run", stub)
    return seen


def test_side_files_are_named_by_the_pattern_and_get_their_headers(tmp_path, captured):
    mod = script()
    pat = str(tmp_path / "side_%s.tsv")
    argv = base_argv(tmp_path, ["-P", pat, "--output-stats=sample_metrics", "--output-stats=segment_metrics"])
    assert mod.main(argv) == 0
    assert sorted(captured["outfiles"]) == ["sample_metrics", "segment_metrics"]
    assert all(f.closed for f in captured["outfiles"].values())
    # gat-run.py's part writes the header of sample_metrics; that of segment_metrics is run()'s (gat/__init__.py:916)
    assert open(pat % "sample_metrics").read() == HEADER
    assert open(pat % "segment_metrics").read() == ""
    # an existing file: refused without --force, overwritten with it
    with pytest.raises(OSError, match="already exists"):
        mod.main(argv)
    open(pat % "sample_metrics", "w").write("stale\n")
    assert mod.main(argv + ["--force"]) == 0
    assert open(pat % "sample_metrics").read() == HEADER
    # one of the two alone
    one = str(tmp_path / "one_%s")
    assert mod.main(base_argv(tmp_path, ["--output-filename-pattern=%s" % one, "--output-stats=segment_metrics"])) == 0
    assert sorted(captured["outfiles"]) == ["segment_metrics"] and not os.path.exists(one % "sample_metrics")


def test_all_opens_neither(tmp_path, captured, monkeypatch):
    """--output-stats=all keeps meaning the collection summaries"""
    from gat_amd import io as IO
    monkeypatch.setattr(IO, "buildSegments", lambda options: (None, None, None, None))      # (its summaries are not this test's)
    monkeypatch.setattr(IO, "applyIsochores", lambda *a, **kw: None)
    mod = script()
    pat = str(tmp_path / "all_%s")
    assert mod.main(base_argv(tmp_path, ["-P", pat, "--output-stats=all"])) == 0
    assert captured["outfiles"] == {}
    assert not os.path.exists(pat % "sample_metrics") and not os.path.exists(pat % "segment_metrics")
    # ... and so does a run without any
    assert mod.main(base_argv(tmp_path, ["-P", pat])) == 0 and captured["outfiles"] == {}


@pytest.mark.parametrize("conditional", [["--conditional=segment-centered", "--conditional-expansion=3"],
                                         ["--conditional=annotation-centered", "--conditional-expansion=2"],
                                         ["--conditional=cooccurance"]], ids=lambda c: c[0].split("=")[1])
def test_sample_metrics_of_a_generated_workspace_are_refused_before_sampling(tmp_path, monkeypatch, conditional):
    import gat_amd
    from gat_amd import _lib

    def no_device(*a, **kw):
        raise AssertionError("a device context was asked for")

    monkeypatch.setattr(_lib, "Context", no_device)
    monkeypatch.setattr(gat_amd, "_sample_start", no_device)
    mod = script()
    pat = str(tmp_path / "c_%s")
    with pytest.raises(NotImplementedError, match="--conditional"):
        mod.main(base_argv(tmp_path, ["-P", pat, "--num-samples=5", "--output-stats=sample_metrics"] + conditional))
    assert open(pat % "sample_metrics").read() == HEADER                     # (nothing but the header)


def test_sample_metrics_on_the_reference_stream_are_refused(tmp_path, monkeypatch):
    from gat_amd import _lib
    monkeypatch.setattr(_lib, "Context", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a device context was asked for")))
    with pytest.raises(NotImplementedError, match="reference-stream"):
        script().main(base_argv(tmp_path, ["-P", str(tmp_path / "r_%s"), "--output-stats=sample_metrics", "--reference-stream",
                                           "--random-seed=3"]))


@pytest.mark.parametrize("name", ["plain", "tracks", "isochores"])
def test_segment_metrics_file_from_the_model_sums(monkeypatch, tmp_path, name):
    """run()'s segment_metrics block (metrics.write_segment_metrics) on the golden runs' inputs, the device's sums replaced by
    the model's: the reference's file, byte for byte -- the keys, their workspaces, the order, the text"""
    import gat_amd
    from gat_amd import _lib, metrics
    from gat_amd import io as IO

    def model_list_metrics(ctx, lists, list_off, n_lists, ws, ws_off, n_groups):
        out = np.zeros((n_lists, n_groups, len(M.WORDS)), dtype=np.int64)
        for l in range(n_lists):
            for g in range(n_groups):
                k = l * n_groups + g
                out[l, g] = M.words_of_array(lists[list_off[k]:list_off[k + 1]], ws[ws_off[g]:ws_off[g + 1]])
        return out

    monkeypatch.setattr(_lib, "list_metrics", model_list_metrics)
    extra = json.load(open(os.path.join(GOLD, "cases.json")))[name]
    opts, _ = gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS).parse_args(base_argv(tmp_path, extra)[1:])
    opts.output_stats = []
    segments, annotations, workspaces, isochores = IO.buildSegments(opts)
    workspace = IO.applyIsochores(segments, annotations, workspaces, opts, isochores)
    out = io.StringIO()
    metrics.write_segment_metrics(out, segments, workspace, ctx=object())
    assert out.getvalue() == open(os.path.join(GOLD, "expected_%s.segment_metrics" % name)).read()


def test_contig_workspace_is_the_union_of_the_isochore_pieces():
    """with isochore keys a contig's samples are measured against the contig's workspace: its pieces merged"""
    from gat_amd import engine, metrics
    from gat_amd import intervals as iv
    w = engine.IntervalDictionary()
    w.add("chr1.a", engine.SegmentList(iter=[(0, 10), (30, 40)], normalize=True))
    w.add("chr1.b", engine.SegmentList(iter=[(10, 20), (50, 60)], normalize=True))
    w.add("chr2.a", engine.SegmentList(iter=[(5, 6)], normalize=True))
    data, off, size = metrics.contig_workspace(w, ["chr2", "chr1", "chrX"])
    assert off.tolist() == [0, 1, 4, 4] and size.tolist() == [1, 40, 0]
    assert list(zip(data["start"].tolist(), data["end"].tolist())) == [(5, 6), (0, 20), (30, 40), (50, 60)]
    # without isochore keys the lists stay as normalize left them: adjacent pieces are two pieces
    w = engine.IntervalDictionary()
    w.add("chr1", engine.SegmentList(iter=[(0, 10), (10, 20)], normalize=True))
    data, off, size = metrics.contig_workspace(w, ["chr1"])
    assert off.tolist() == [0, 2] and size.tolist() == [20] and len(iv.EMPTY) == 0
