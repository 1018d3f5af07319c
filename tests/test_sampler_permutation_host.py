"""CPU: the global permutation sampler's host side -- the command line, the Python class and the C ABI's constants."""
import os

import pytest

import gat_amd
from gat_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gat_mi355.h")


def test_parser_takes_global_permutation():
    opts, _ = gat_amd.buildParser().parse_args(["-m", "global-permutation"])
    assert opts.sampler == "global-permutation"
    for other in ("local-permutation", "uniform", "brute-force"):      # (still outside the accelerated path)
        with pytest.raises(SystemExit):
            gat_amd.buildParser().parse_args(["-m", other])


def test_sampler_global_permutation_class():
    s = gat_amd.SamplerGlobalPermutation()
    assert s.kind == 3 and isinstance(s, gat_amd.Sampler)
    assert gat_amd.engine.SamplerGlobalPermutation is gat_amd.SamplerGlobalPermutation


def test_from_segments_maps_the_sampler():
    opts, _ = gat_amd.buildParser().parse_args(["--sampler=global-permutation"])
    assert type(gat_amd.sampler_from_options(opts)) is gat_amd.SamplerGlobalPermutation  # (what fromSegments calls)


def test_reference_stream_refused():
    """run(reference_stream=True) with SamplerGlobalPermutation raises before anything reaches a device."""
    e = gat_amd.IntervalCollection()
    with pytest.raises(NotImplementedError):
        gat_amd.run(e, e, e, gat_amd.SamplerGlobalPermutation(), [gat_amd.CounterNucleotideOverlap()],
                    workspace_generator=gat_amd.UnconditionalWorkspace(), num_samples=4, random_seed=1, reference_stream=True)


def test_ctypes_constants_match_header():
    text = open(HEADER).read()
    for name in ("ANNOTATOR", "SEGMENTS", "SHIFT", "GLOBAL_PERMUTATION"):
        assert "#define GAT_SAMPLER_%s %d " % (name, getattr(_lib, "SAMPLER_" + name)) in text, name
    assert _lib.SAMPLER_GLOBAL_PERMUTATION == 3 == gat_amd.SamplerGlobalPermutation.kind
