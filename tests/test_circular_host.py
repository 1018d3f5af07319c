"""CPU: the circular sampler's host side -- its tables at problem creation (tests/host/circular_check.cpp, a stand-alone
program compiled for the host alone with the address and undefined-behaviour sanitizers), the command line, the Python
class and the C ABI's constants."""
import os
import shutil
import subprocess

import pytest

import gat_amd
from gat_amd import _lib, coverage, enrichment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gat_mi355.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_circular_check(tmp_path):
    """the linear tables of hand-made and random units, the slab capacity n + |W|, the unit without a working segment"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path / "circular_check")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "gat_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "circular_check.cpp"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, "the check program does not compile:\n" + c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "circular_check failed (exit status %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])


def test_tool_parsers_take_circular():
    """every tool script's parser takes --sampler=circular"""
    import importlib.util
    for tool in ("gat-run", "gat-coverage", "gat-distance", "gat-signal", "gat-local", "gat-pairs", "gat-geneset", "gat-profile"):
        src = open(os.path.join(ROOT, "scripts", tool + ".py")).read()
        assert "TOOL_SAMPLERS" in src, tool
    spec = importlib.util.spec_from_file_location("gat_run_cli_circular_host", os.path.join(ROOT, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}

    class Reached(Exception):
        pass

    def stop(options, args=None):
        seen["sampler"] = options.sampler
        raise Reached()

    old = gat_amd.fromSegments
    gat_amd.fromSegments = stop
    try:
        with pytest.raises(Reached):
            mod.main(["gat-run.py", "--sampler=circular", "--segments=s.bed", "--annotations=a.bed", "--workspace=w.bed"])
    finally:
        gat_amd.fromSegments = old
    assert seen["sampler"] == "circular"


def test_samplers_are_mapped():
    opts, _ = gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS).parse_args(["--sampler=circular"])
    assert type(gat_amd.sampler_from_options(opts)) is gat_amd.SamplerCircular          # (what fromSegments calls)

    class Opt(object):
        sampler = "circular"
    assert isinstance(coverage.make_sampler(Opt()), gat_amd.SamplerCircular)
    assert gat_amd.SamplerCircular in coverage.SAMPLERS and enrichment.SAMPLERS is coverage.SAMPLERS


def test_reference_stream_refused():
    """run(reference_stream=True) with SamplerCircular raises before anything reaches a device."""
    e = gat_amd.IntervalCollection()
    with pytest.raises(NotImplementedError, match="SamplerCircular runs on the per-unit streams only"):
        gat_amd.run(e, e, e, gat_amd.SamplerCircular(), [gat_amd.CounterNucleotideOverlap()],
                    workspace_generator=gat_amd.UnconditionalWorkspace(), num_samples=4, random_seed=1, reference_stream=True)


def test_ctypes_constant_matches_header():
    text = open(HEADER).read()
    assert "#define GAT_SAMPLER_CIRCULAR %d " % _lib.SAMPLER_CIRCULAR in text
    assert _lib.SAMPLER_CIRCULAR == 6 == gat_amd.SamplerCircular.kind
