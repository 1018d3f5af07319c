"""CPU: the registry of samplers (gat_amd/engine.py: SAMPLER_CLASSES and the helpers beside it) -- options to class, the
fields a sampler adds to a flat problem, the ids and names against the C headers, what is refused and with which words, and
sample() on empty input: no device, one draw of the right generator."""
import os
import random
import re

import numpy as np
import pytest

import gat_amd
from gat_amd import _lib, coverage, engine, enrichment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = engine.SAMPLER_CLASSES
LIST_SAMPLERS = [cls for cls in CLASSES if cls not in (gat_amd.SamplerAnnotator, gat_amd.SamplerSegments)]
PYTHON_SEEDED = (gat_amd.SamplerGlobalPermutation, gat_amd.SamplerLocalPermutation)

# word, class, and -- for an instance with the parameters of `build` -- the fields it adds to a flat problem
CASES = [
    ("annotator", gat_amd.SamplerAnnotator, dict(bucket_size=4, nbuckets=77), dict(sampler=0, bucket_size=4, nbuckets=77)),
    ("segments", gat_amd.SamplerSegments, dict(bucket_size=3, nbuckets=9), dict(sampler=1, bucket_size=3, nbuckets=9)),
    ("shift", gat_amd.SamplerShift, dict(radius=3.5, extension=40), dict(sampler=2, shift_radius=3.5, shift_extension=40)),
    ("global-permutation", gat_amd.SamplerGlobalPermutation, {}, dict(sampler=3)),
    ("local-permutation", gat_amd.SamplerLocalPermutation, {}, dict(sampler=4)),
    ("brute-force", gat_amd.SamplerBruteForce, dict(ntries_inner=7, ntries_outer=3, bucket_size=2, nbuckets=50),
     dict(sampler=5, bucket_size=2, nbuckets=50, brute_ntries_inner=7, brute_ntries_outer=3)),
    ("circular", gat_amd.SamplerCircular, {}, dict(sampler=6)),
    ("universe", gat_amd.SamplerUniverse, {}, dict(sampler=7)),
]
IDS = [c[0] for c in CASES]
SAMPLER_KEYS = ("sampler", "bucket_size", "nbuckets", "shift_radius", "shift_extension", "brute_ntries_inner", "brute_ntries_outer")


def parse(*args):
    return gat_amd.buildParser(samplers=gat_amd.TOOL_SAMPLERS + gat_amd.UNIVERSE_SAMPLERS).parse_args(list(args))[0]


def test_the_registry_is_the_eight_classes():
    assert [c[1] for c in CASES] == list(CLASSES) and coverage.SAMPLERS is CLASSES and enrichment.SAMPLERS is CLASSES
    assert tuple(cls.word for cls in CLASSES) == gat_amd.TOOL_SAMPLERS + gat_amd.UNIVERSE_SAMPLERS == tuple(IDS)
    assert [cls.kind for cls in CLASSES] == list(range(8))
    assert all(issubclass(cls, gat_amd.Sampler) for cls in CLASSES)
    assert gat_amd.SAMPLERS == ("annotator", "segments", "shift", "global-permutation")
    assert gat_amd.ALL_SAMPLERS == gat_amd.SAMPLERS + ("local-permutation",)
    assert gat_amd.CLI_SAMPLERS == gat_amd.ALL_SAMPLERS + ("brute-force",)
    assert gat_amd.TOOL_SAMPLERS == gat_amd.CLI_SAMPLERS + ("circular",) and gat_amd.UNIVERSE_SAMPLERS == ("universe",)


@pytest.mark.parametrize("word,cls,build,fields", CASES, ids=IDS)
def test_options_build_the_class(word, cls, build, fields):
    opts = parse("--sampler=" + word, "--bucket-size=6", "--nbuckets=321", "--shift-expansion=1.5", "--shift-extension=12")
    for make in (gat_amd.sampler_from_options, engine.sampler_from_options, coverage.make_sampler, enrichment.make_sampler):
        s = make(opts)
        assert type(s) is cls
        want = {"annotator": dict(bucket_size=6, nbuckets=321, nunsuccessful_rounds=0),
                "segments": dict(bucket_size=1, nbuckets=100000),                  # (no bucket arguments: the class's defaults)
                "shift": dict(radius=1.5, extension=12),
                "brute-force": dict(bucket_size=1, nbuckets=100000, ntries_inner=100, ntries_outer=10)}.get(word, {})
        assert vars(s) == want


def test_an_unknown_word_is_refused():
    class Opt(object):
        sampler = "uniform"
    for make in (gat_amd.sampler_from_options, coverage.make_sampler):
        with pytest.raises(ValueError, match="sampler 'uniform' is outside the accelerated path"):
            make(Opt())


def two_units():
    segs, ws = gat_amd.IntervalDictionary(), gat_amd.IntervalDictionary()
    for contig, at in (("chr1", 100), ("chr2", 300)):
        segs.add(contig, gat_amd.SegmentList(iter=[(at, at + 10), (at + 40, at + 50)], normalize=True))
        ws.add(contig, gat_amd.SegmentList(iter=[(0, 1000)], normalize=True))
    return segs, ws


@pytest.mark.parametrize("word,cls,build,fields", CASES, ids=IDS)
def test_flat_fields(word, cls, build, fields):
    s = cls(**build)
    assert s.flat_fields() == fields
    flat, sa, wa = coverage.flatten(*two_units(), s)
    assert flat["n_units"] == 2
    # (flatten_units is handed the sampler's buckets, 0 / 100000 for a class without them)
    assert dict((k, flat[k]) for k in SAMPLER_KEYS if k in flat) == dict(dict(bucket_size=0, nbuckets=100000), **fields)
    assert enrichment.flatten is coverage.flatten


def test_ids_and_names_match_the_headers():
    defines = dict((m.group(1), int(m.group(2))) for m in
                   re.finditer(r"^#define (GAT_SAMPLER_[A-Z_]+) (\d+)\s", open(os.path.join(ROOT, "include", "gat_mi355.h")).read(), re.M))
    table = re.findall(r'^\s*\{(GAT_SAMPLER_[A-Z_]+), "(\w+)", (true|false), (true|false)\},$',
                       open(os.path.join(ROOT, "gat_amd", "csrc", "gat_samplers.h")).read(), re.M)
    assert len(table) == 8 == len(set(define for define, _, _, _ in table))
    for cls, (define, name, wave_per_unit, _) in zip(CLASSES, table):
        assert name == cls.__name__
        assert defines[define] == cls.kind == getattr(_lib, define[len("GAT_"):])
        assert (wave_per_unit == "true") == (not cls.has_reference_stream)          # (a wave per unit: per-unit streams only)


def run_on_nothing(sampler, **kwargs):
    e = gat_amd.IntervalCollection()
    return gat_amd.run(e, e, e, sampler, [gat_amd.CounterNucleotideOverlap()], workspace_generator=gat_amd.UnconditionalWorkspace(),
                       num_samples=4, random_seed=1, **kwargs)


@pytest.mark.parametrize("cls", LIST_SAMPLERS, ids=[c.word for c in LIST_SAMPLERS])
def test_reference_stream_refused(cls):
    with pytest.raises(NotImplementedError, match="^reference_stream: %s runs on the per-unit streams only$" % cls.__name__):
        run_on_nothing(cls(), reference_stream=True)

    class Derived(cls):
        pass
    with pytest.raises(NotImplementedError, match="^reference_stream: %s runs on the per-unit streams only$" % cls.__name__):
        run_on_nothing(Derived(), reference_stream=True)


@pytest.mark.parametrize("cls", [gat_amd.SamplerAnnotator, gat_amd.SamplerSegments], ids=["annotator", "segments"])
def test_reference_stream_taken(cls, monkeypatch):
    """the run goes on past the check, as far as asking for a device"""
    class Reached(Exception):
        pass

    def reached(*args, **kwargs):
        raise Reached()
    monkeypatch.setattr(engine, "get_context", reached)
    monkeypatch.setattr(gat_amd, "get_context", reached)
    assert cls.has_reference_stream
    engine.check_reference_stream(cls())
    with pytest.raises(Reached):
        run_on_nothing(cls(), reference_stream=True)


class Foreign(gat_amd.Sampler):
    kind = 0

    def sample(self, segments, workspace, seed=None):
        return segments


@pytest.mark.parametrize("sampler", [Foreign(), object(), None], ids=["subclass", "object", "none"])
def test_foreign_samplers_are_refused(sampler):
    names = [cls.__name__ for cls in CLASSES]
    message = "^only %s and %s run on the GPU path$" % (", ".join(names[:-1]), names[-1])
    assert message == ("^only SamplerAnnotator, SamplerSegments, SamplerShift, SamplerGlobalPermutation, SamplerLocalPermutation, "
                       "SamplerBruteForce, SamplerCircular and SamplerUniverse run on the GPU path$")
    segs, ws = two_units()
    with pytest.raises(NotImplementedError, match=message):
        run_on_nothing(sampler)
    with pytest.raises(NotImplementedError, match=message):
        coverage.sample_coverage(segs, ws, sampler, 4, 10, random_seed=1)
    with pytest.raises(NotImplementedError, match=message):
        enrichment.track_start(segs, ws, sampler, 4, 1)


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_sample_of_nothing_draws_one_seed_and_makes_no_context(cls, monkeypatch):
    def no_context(*args, **kwargs):
        raise AssertionError("sample() of an empty list asked for a context")
    monkeypatch.setattr(engine, "get_context", no_context)
    monkeypatch.setattr(_lib, "Problem", no_context)
    workspace = gat_amd.SegmentList(iter=[(0, 100)], normalize=True)
    np_saved, py_saved = np.random.get_state(), random.getstate()
    try:
        for segments, ws in ((gat_amd.SegmentList(), workspace), (workspace, gat_amd.SegmentList())):
            np.random.seed(77)
            random.seed(78)
            np_before, py_before = np.random.get_state(), random.getstate()
            got = cls().sample(segments, ws, seed=None)
            np_after, py_after = np.random.get_state(), random.getstate()
            assert type(got) is gat_amd.SegmentList and len(got) == 0
            np.random.seed(77)
            random.seed(78)
            if cls in PYTHON_SEEDED:
                random.getrandbits(32)
            else:
                np.random.randint(0, 2 ** 32)
            assert same_state(np_after, np.random.get_state()) and py_after == random.getstate()
            assert same_state(np_after, np_before) == (cls in PYTHON_SEEDED) and (py_after == py_before) == (cls not in PYTHON_SEEDED)
            # a seed given: neither generator moves
            np_before, py_before = np.random.get_state(), random.getstate()
            assert len(cls().sample(segments, ws, seed=5)) == 0
            assert same_state(np_before, np.random.get_state()) and py_before == random.getstate()
    finally:
        np.random.set_state(np_saved)
        random.setstate(py_saved)


def test_segments_off_the_workspace():
    """an empty overlap with the workspace returns early for every sampler but local-permutation (it goes on to the device);
    only the annotator insists on normalized segments"""
    assert [cls.empty_overlap_returns for cls in CLASSES] == [True, True, True, True, False, True, True, True]
    away = gat_amd.SegmentList(iter=[(500, 600)], normalize=True)
    workspace = gat_amd.SegmentList(iter=[(0, 100)], normalize=True)
    for cls in CLASSES:
        if cls.empty_overlap_returns:
            assert len(cls().sample(away, workspace, seed=1)) == 0
    unsorted = gat_amd.SegmentList(iter=[(50, 60), (10, 20)])
    assert not unsorted.isNormalized
    with pytest.raises(AssertionError, match="segment list is not normalized"):
        gat_amd.SamplerAnnotator().sample(unsorted, workspace, seed=1)
    for cls in CLASSES:
        with pytest.raises(AssertionError, match="workspace is not normalized"):
            cls().sample(workspace, unsorted, seed=1)
