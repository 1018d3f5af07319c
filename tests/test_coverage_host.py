"""CPU: gat-coverage's host side -- the command line parses and refuses what it should, the module imports without a
device, the host's per-bin bases equal the model's, the rows written are the bins with a workspace or a sampled base."""
import importlib.util
import io
import os

import numpy as np
import pytest

import coverage_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def script():
    spec = importlib.util.spec_from_file_location("gat_coverage_cli", os.path.join(ROOT, "scripts", "gat-coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parser_defaults_and_options():
    import gat_amd
    opts, args = script().buildParser().parse_args(
        ["--segments=a.bed", "--workspace=w.bed", "--isochores=i.bed", "--with-segment-tracks", "--sampler=brute-force",
         "--shift-expansion=3", "--shift-extension=7", "--bucket-size=2", "--nbuckets=50", "--num-samples=20", "--random-seed=4",
         "--bin-size=64", "--device=1", "--stdout=o.tsv", "--log=l.txt", "--verbose=0"])
    assert args == [] and opts.segment_files == ["a.bed"] and opts.workspace_files == ["w.bed"] and opts.isochore_files == ["i.bed"]
    assert opts.ignore_segment_tracks is False and opts.sampler == "brute-force" and opts.bin_size == 64 and opts.num_samples == 20
    assert (opts.shift_expansion, opts.shift_extension, opts.bucket_size, opts.nbuckets) == (3.0, 7.0, 2, 50)
    assert (opts.random_seed, opts.device, opts.stdout, opts.stdlog, opts.loglevel) == (4, 1, "o.tsv", "l.txt", 0)
    opts, _ = script().buildParser().parse_args([])
    assert opts.bin_size == 1000 and opts.sampler == "annotator" and opts.ignore_segment_tracks is True
    for name in gat_amd.CLI_SAMPLERS:
        assert script().buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name


def test_unknown_sampler_is_refused(capsys):
    with pytest.raises(SystemExit):
        script().buildParser().parse_args(["--sampler=uniform"])
    assert "invalid choice" in capsys.readouterr().err
    with pytest.raises(SystemExit):                      # annotations are none of this script's inputs
        script().buildParser().parse_args(["--annotations=a.bed"])


def test_module_imports_without_a_device():
    from gat_amd import coverage
    assert callable(coverage.sample_coverage) and coverage.HEADER[0] == "track" and coverage.HEADER[-1] == "depth"


def test_inputs_without_annotations():
    """the golden command-line inputs prepared without an annotation file: tracks, isochore keys, a problem of no tracks"""
    from gat_amd import coverage
    mod = script()
    base = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--workspace=%s" % os.path.join(CLI, "workspace.bed")]
    opts, _ = mod.buildParser().parse_args(base)
    segments, workspace = coverage.build_inputs(opts)
    assert list(segments.tracks) == ["merged"]
    flat, _, _ = coverage.flatten(segments["merged"], workspace, coverage.make_sampler(opts))
    assert flat["n_tracks"] == 0 and flat["merge_contigs"] == 0 and flat["n_contigs"] == 4
    opts, _ = mod.buildParser().parse_args(base + ["--with-segment-tracks", "--isochores=%s" % os.path.join(CLI, "isochores.bed")])
    segments, workspace = coverage.build_inputs(opts)
    assert len(segments.tracks) == 2
    flat, _, _ = coverage.flatten(segments[list(segments.tracks)[0]], workspace, coverage.make_sampler(opts))
    assert flat["merge_contigs"] == 1 and flat["n_units"] > flat["n_contigs"]
    with pytest.raises(ValueError):
        coverage.build_inputs(mod.buildParser().parse_args(["--segments=%s" % os.path.join(CLI, "segments.bed")])[0])


def test_bin_bases_equals_the_model():
    from gat_amd import coverage, intervals
    r = np.random.RandomState(3)
    for _ in range(60):
        n = int(r.choice([0, 1, 20]))
        a = intervals.make(r.randint(0, 500, n), 0)
        a["end"] = a["start"] + r.randint(0, 120, n)
        bin_size, n_bins = int(r.choice([1, 7, 64, 1000])), int(r.choice([0, 1, 5, 100]))
        got = coverage.bin_bases(a, bin_size, n_bins)
        assert got.dtype == np.int64 and np.array_equal(got, M.coverage(a, bin_size, n_bins)[0])


def test_rows_are_the_bins_with_a_workspace_or_sampled_base():
    from gat_amd import coverage
    cov = coverage.Coverage(["c1", "c2"], 10, 4)
    z = lambda *v: np.array(v, dtype=np.int64)      # noqa: E731
    cov.workspace_bases = {"c1": z(10, 0, 0, 3), "c2": z(0)}
    cov.segment_bases = {"c1": z(2, 0, 0, 0), "c2": z(0)}
    cov.bases = {"c1": z(7, 0, 5, 0), "c2": z(0)}
    cov.starts = {"c1": z(1, 0, 1, 0), "c2": z(0)}
    cov.ends = {"c1": z(0, 0, 2, 0), "c2": z(0)}
    cov.outside = {"c1": 0, "c2": 12}
    out = io.StringIO()
    coverage.write_rows(out, "t", cov)
    lines = out.getvalue().splitlines()
    assert [l.split("\t")[:9] for l in lines[:3]] == [["t", "c1", "0", "10", "10", "2", "7", "1", "0"],
                                                       ["t", "c1", "20", "30", "0", "0", "5", "1", "2"],
                                                       ["t", "c1", "30", "40", "3", "0", "0", "0", "0"]]
    assert [float(l.split("\t")[9]) for l in lines[:3]] == [7 / 40.0, 5 / 40.0, 0.0]
    assert lines[3:] == ["# t\tc2\t12"]
