"""CPU: the brute-force sampler's host side -- the command line, the Python class, the C ABI's constants and structures."""
import ctypes
import os

import pytest

import gat_amd
from gat_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "gat_mi355.h")


def test_sampler_tuples():
    """SAMPLERS and ALL_SAMPLERS stay as they were; CLI_SAMPLERS adds brute-force; uniform is in none of them."""
    assert gat_amd.SAMPLERS == ("annotator", "segments", "shift", "global-permutation")
    assert gat_amd.ALL_SAMPLERS == gat_amd.SAMPLERS + ("local-permutation",)
    assert gat_amd.CLI_SAMPLERS == gat_amd.ALL_SAMPLERS + ("brute-force",)


def test_parser_takes_brute_force():
    for arg in (["-m", "brute-force"], ["--sampler=brute-force"]):
        opts, _ = gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS).parse_args(arg)
        assert opts.sampler == "brute-force"
    for parser in (gat_amd.buildParser(), gat_amd.buildParser(samplers=gat_amd.ALL_SAMPLERS)):
        with pytest.raises(SystemExit):
            parser.parse_args(["-m", "brute-force"])
    for samplers in (gat_amd.SAMPLERS, gat_amd.ALL_SAMPLERS, gat_amd.CLI_SAMPLERS):
        with pytest.raises(SystemExit):
            gat_amd.buildParser(samplers=samplers).parse_args(["-m", "uniform"])


def test_script_parses_brute_force(tmp_path):
    """scripts/gat-run.py gets past its option parser with -m brute-force and hands the options to fromSegments."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gat_run_cli_brute_host", os.path.join(HERE, "..", "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit) as e:
        mod.main(["gat-run.py", "--sampler=uniform"])
    assert e.value.code == 2
    seen = {}

    class Reached(Exception):
        pass

    def stop(options, args=None):
        seen["sampler"] = options.sampler
        raise Reached()

    saved = gat_amd.fromSegments
    gat_amd.fromSegments = stop
    try:
        with pytest.raises(Reached):
            mod.main(["gat-run.py", "-m", "brute-force", "--log=%s" % str(tmp_path / "log")])
    finally:
        gat_amd.fromSegments = saved
    assert seen == {"sampler": "brute-force"}


def test_sampler_brute_force_class():
    s = gat_amd.SamplerBruteForce()
    assert s.kind == 5 and isinstance(s, gat_amd.Sampler)
    assert (s.bucket_size, s.nbuckets, s.ntries_inner, s.ntries_outer) == (1, 100000, 100, 10)
    assert gat_amd.engine.SamplerBruteForce is gat_amd.SamplerBruteForce
    t = gat_amd.SamplerBruteForce(bucket_size=7, nbuckets=50, ntries_inner=3, ntries_outer=2)
    assert (t.bucket_size, t.nbuckets, t.ntries_inner, t.ntries_outer) == (7, 50, 3, 2)


def test_negative_tries_refused():
    for kw in (dict(ntries_inner=-1), dict(ntries_outer=-3)):
        with pytest.raises(ValueError):
            gat_amd.SamplerBruteForce(**kw)


def test_from_segments_builds_the_class(monkeypatch):
    """fromSegments with --sampler=brute-force hands run() a SamplerBruteForce with the reference's defaults -- bucket_size
    1 whatever --bucket-size says (scripts/gat-run.py:139-140 of the reference passes nothing)."""
    cli = os.path.join(HERE, "golden", "cli")
    opts, _ = gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS).parse_args(
        ["--segments=%s" % os.path.join(HERE, "golden", "brute_force", "cli", "segments.bed"),
         "--annotations=%s" % os.path.join(cli, "annotations.bed"), "--workspace=%s" % os.path.join(cli, "workspace.bed"),
         "--sampler=brute-force", "--bucket-size=9"])
    seen = {}

    def fake_run(segments, annotations, workspace, sampler, counters, **kw):
        seen["sampler"] = sampler
        return []

    monkeypatch.setattr(gat_amd, "run", fake_run)
    gat_amd.fromSegments(opts)
    s = seen["sampler"]
    assert type(s) is gat_amd.SamplerBruteForce
    assert (s.bucket_size, s.nbuckets, s.ntries_inner, s.ntries_outer) == (1, 100000, 100, 10)


def test_reference_stream_refused():
    """run(reference_stream=True) with SamplerBruteForce raises before anything reaches a device."""
    e = gat_amd.IntervalCollection()
    with pytest.raises(NotImplementedError):
        gat_amd.run(e, e, e, gat_amd.SamplerBruteForce(), [gat_amd.CounterNucleotideOverlap()],
                    workspace_generator=gat_amd.UnconditionalWorkspace(), num_samples=4, random_seed=1, reference_stream=True)


def test_ctypes_match_header():
    text = open(HEADER).read()
    assert "#define GAT_SAMPLER_BRUTE_FORCE %d " % _lib.SAMPLER_BRUTE_FORCE in text
    assert _lib.SAMPLER_BRUTE_FORCE == 5 == gat_amd.SamplerBruteForce.kind
    # the new fields stand at the end of their structures, in the header's order
    assert [f for f, _ in _lib.ProblemDesc._fields_][-2:] == ["brute_ntries_inner", "brute_ntries_outer"]
    assert [f for f, _ in _lib.Stats._fields_][-2:] == ["n_restarts", "n_unconverged"]
    desc = text[text.index("typedef struct {"):text.index("} gat_problem_desc;")]
    assert desc.rstrip().endswith("int32_t brute_ntries_outer;") and "int32_t brute_ntries_inner;" in desc
    stats = text[text.index("int64_t n_empty_windows;"):text.index("} gat_stats;")]
    assert stats.index("int64_t n_restarts;") < stats.index("int64_t n_unconverged;")
    assert all(t is ctypes.c_int32 for _, t in _lib.ProblemDesc._fields_[-2:])
