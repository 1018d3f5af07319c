"""CPU: the local permutation sampler's host side -- the command line, the Python class, the C ABI's constants and what
problem creation derives per unit (local_permutation_model.unit_tables on the hand-made shapes)."""
import inspect
import os

import pytest

import gat_amd
import local_permutation_model as M
from gat_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gat_mi355.h")


def test_parser_takes_local_permutation():
    """the command line's parser (scripts/gat-run.py builds it with ALL_SAMPLERS) takes --sampler=local-permutation."""
    assert "local-permutation" in gat_amd.ALL_SAMPLERS and set(gat_amd.SAMPLERS) < set(gat_amd.ALL_SAMPLERS)
    for arg in (["-m", "local-permutation"], ["--sampler=local-permutation"]):
        opts, _ = gat_amd.buildParser(samplers=gat_amd.ALL_SAMPLERS).parse_args(arg)
        assert opts.sampler == "local-permutation"
    for other in ("uniform", "brute-force"):                            # (still outside the accelerated path)
        with pytest.raises(SystemExit):
            gat_amd.buildParser(samplers=gat_amd.ALL_SAMPLERS).parse_args(["-m", other])


def test_script_parses_local_permutation(tmp_path):
    """scripts/gat-run.py gets past its option parser with --sampler=local-permutation: the run ends on the missing
    input files, not with the parser's exit status 2."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("gat_run_cli_host", os.path.join(here, "..", "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit) as e:
        mod.main(["gat-run.py", "--sampler=no-such-sampler"])
    assert e.value.code == 2
    # past the parser, main() hands the options to fromSegments: caught there
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
            mod.main(["gat-run.py", "--sampler=local-permutation", "--log=%s" % str(tmp_path / "log")])
    finally:
        gat_amd.fromSegments = saved
    assert seen == {"sampler": "local-permutation"}


def test_sampler_local_permutation_class():
    s = gat_amd.SamplerLocalPermutation()
    assert s.kind == 4 and isinstance(s, gat_amd.Sampler)
    assert gat_amd.engine.SamplerLocalPermutation is gat_amd.SamplerLocalPermutation


def test_from_segments_builds_the_class(monkeypatch):
    """fromSegments on the small CLI inputs with --sampler=local-permutation hands run() a SamplerLocalPermutation."""
    cli = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli")
    opts, _ = gat_amd.buildParser(samplers=gat_amd.ALL_SAMPLERS).parse_args(
        ["--segments=%s" % os.path.join(cli, "segments.bed"), "--annotations=%s" % os.path.join(cli, "annotations.bed"),
         "--workspace=%s" % os.path.join(cli, "workspace.bed"), "--sampler=local-permutation"])
    seen = {}

    def fake_run(segments, annotations, workspace, sampler, counters, **kw):
        seen["sampler"] = sampler
        return []

    monkeypatch.setattr(gat_amd, "run", fake_run)
    gat_amd.fromSegments(opts)
    assert type(seen["sampler"]) is gat_amd.SamplerLocalPermutation


def test_flat_carries_the_kind():
    import local_permutation_edges as LE
    flat = LE.units_flat([([(10, 20)], [(100, 200)])])
    assert flat["sampler"] == 4 == LE.LOCAL


def test_reference_stream_refused():
    """run(reference_stream=True) with SamplerLocalPermutation raises before anything reaches a device."""
    e = gat_amd.IntervalCollection()
    with pytest.raises(NotImplementedError):
        gat_amd.run(e, e, e, gat_amd.SamplerLocalPermutation(), [gat_amd.CounterNucleotideOverlap()],
                    workspace_generator=gat_amd.UnconditionalWorkspace(), num_samples=4, random_seed=1, reference_stream=True)


def test_ctypes_constants_match_header():
    text = open(HEADER).read()
    assert "#define GAT_SAMPLER_LOCAL_PERMUTATION %d " % _lib.SAMPLER_LOCAL_PERMUTATION in text
    assert _lib.SAMPLER_LOCAL_PERMUTATION == 4 == gat_amd.SamplerLocalPermutation.kind


def test_unit_tables_on_the_hand_made_shapes():
    """(first, n, work_start, work_end, free) per active piece."""
    T = M.unit_tables
    assert T([(500, 510)], [(100, 200)]) == []                                   # every segment beyond the workspace
    assert T([(10, 20)], [(100, 200)]) == [(0, 1, 0, 200, 190)]                  # the segment in front of the piece
    assert T([(10, 20)], [(0, 5), (100, 200), (300, 310)]) == [(0, 1, 0, 200, 190), (0, 1, 0, 310, 300)]   # idle, then two
    assert T([(100, 110), (150, 160)], [(90, 200), (300, 400)]) == [(0, 2, 0, 200, 180), (1, 1, 0, 400, 390)]
    assert T([(10, 20), (200, 230)], [(50, 200), (200, 260)]) == [(0, 2, 0, 200, 160), (1, 1, 0, 260, 230)]   # a start AT the end
    assert T([(50, 60)], [(50, 100)]) == [(0, 1, 0, 100, 90)]
    assert T([(0, 40), (40, 100)], [(0, 100)]) == [(0, 2, 0, 100, 0)]            # free = 0
    assert T([(0, 40), (40, 101)], [(0, 100)]) == [(0, 2, 0, 100, -1)]           # the reference raises
    assert T([], [(0, 100)]) == [] and T([(1, 2)], []) == []
