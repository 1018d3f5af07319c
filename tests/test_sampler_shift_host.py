"""CPU: the shift sampler's host side -- the command line, the Python class and the C ABI's structures."""
import os
import re

import pytest

import gat_amd
from gat_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gat_mi355.h")


def test_parser_shift_options_and_defaults():
    parser = gat_amd.buildParser()
    opts, _ = parser.parse_args([])
    assert opts.shift_expansion == 2.0 and opts.shift_extension == 0
    opts, _ = parser.parse_args(["-m", "shift", "--shift-expansion=0.5", "--shift-extension=500.0"])
    assert opts.sampler == "shift" and opts.shift_expansion == 0.5 and opts.shift_extension == 500.0


def test_sampler_shift_class():
    s = gat_amd.SamplerShift()
    assert s.kind == 2 and s.radius == 2.0 and s.extension == 0
    s = gat_amd.SamplerShift(radius=0.5, extension=500.9)      # a float extension truncates, as the reference's cdef int
    assert s.radius == 0.5 and s.extension == 500
    for bad in (dict(radius=-1), dict(extension=-2), dict(radius=float("nan"))):
        with pytest.raises(ValueError):
            gat_amd.SamplerShift(**bad)


def test_reference_stream_refused():
    """run(reference_stream=True) with SamplerShift raises before anything reaches a device."""
    e = gat_amd.IntervalCollection()
    with pytest.raises(NotImplementedError):
        gat_amd.run(e, e, e, gat_amd.SamplerShift(), [gat_amd.CounterNucleotideOverlap()],
                    workspace_generator=gat_amd.UnconditionalWorkspace(), num_samples=4, random_seed=1, reference_stream=True)


def _struct_fields(name):
    text = open(HEADER).read()
    body = dict((m.group(2), m.group(1)) for m in re.finditer(r"typedef struct \{([^{}]*)\} (\w+);", text))[name]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(\w+)\s*;", body)]


def test_ctypes_structures_match_header():
    assert [f for f, _ in _lib.ProblemDesc._fields_] == _struct_fields("gat_problem_desc")
    assert [f for f, _ in _lib.Stats._fields_] == _struct_fields("gat_stats")
    assert "#define GAT_SAMPLER_SHIFT 2" in open(HEADER).read()
