"""CPU: gat-compare's host side -- the command line, which pairs are compared and in which order, the errors, the numpy
path against the reference's tables (tests/golden/compare, tests/golden/make_goldens_compare.py), and the C ABI's
declaration of gat_compare_stats against the ctypes signature."""
import ctypes
import os
import re

import numpy as np
import pytest

import compare_tables as T
import gat_amd
from gat_amd import _lib
from gat_amd import compare as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gat_mi355.h")


def _rows(names, n_samples=20, seed=1, track=None):
    """AnnotatorResults as fromCounts makes them; names: (track, annotation) or annotation (with `track`)"""
    rs = np.random.RandomState(seed)
    out = []
    for name in names:
        t, a = (track, name) if track is not None else name
        out.append(gat_amd.AnnotatorResult(t, a, "na", float(rs.randint(100, 4000)), rs.randint(50, 5000, n_samples).astype(np.float64)))
    return out


def test_parser_options_and_defaults():
    mod = T.script()
    opts, args = mod.buildParser().parse_args(["a.tsv", "b.tsv"])
    assert args == ["a.tsv", "b.tsv"]
    assert (opts.output_order, opts.pvalue_method, opts.qvalue_method, opts.qvalue_lambda, opts.qvalue_pi0_method, opts.pseudo_count,
            opts.input_filename_descriptions) == ("observed", "empirical", "BH", None, "smoother", 1.0, None)
    opts, args = mod.buildParser().parse_args(["--order=pvalue", "-p", "norm", "-q", "storey", "--qvalue-lambda=0.5",
                                               "--qvalue-pi0-method=bootstrap", "--descriptions=d.tsv", "--pseudo-count=0.5", "x"])
    assert (opts.output_order, opts.pvalue_method, opts.qvalue_method, opts.qvalue_lambda, opts.qvalue_pi0_method, opts.pseudo_count,
            opts.input_filename_descriptions, args) == ("pvalue", "norm", "storey", 0.5, "bootstrap", 0.5, "d.tsv", ["x"])
    for bad in (["--order=nothing"], ["--qvalue-method=fdr"], ["--output-plots-pattern=%s.png"]):    # (plots: as gat-run.py here)
        with pytest.raises(SystemExit) as e:
            mod.buildParser().parse_args(bad)
        assert e.value.code == 2
    run_mod_spec = os.path.join(ROOT, "scripts", "gat-run.py")
    assert "output-plots-pattern" not in open(run_mod_spec).read()


def test_single_file_pairs_are_the_combinations_in_order():
    rows = _rows(["a3", "a1", "a2", "a0"], track="merged")
    pairs = C.pairs_of([rows])
    assert [(p.track, p.annotation) for p in pairs] == [("a3", "a1"), ("a3", "a2"), ("a3", "a0"), ("a1", "a2"), ("a1", "a0"), ("a2", "a0")]
    assert all(p.data1.annotation == p.track and p.data2.annotation == p.annotation for p in pairs)
    res = C.compare([rows])
    assert [(r.track, r.annotation, r.counter) for r in res] == [(p.track, p.annotation, "na") for p in pairs]
    for r, p in zip(res, pairs):
        assert r.observed == p.data2.fold - p.data1.fold and r.nsamples == 20


def test_several_files_walk_shared_tracks_and_annotations_sorted():
    f0 = _rows([("tB", "y"), ("tB", "x"), ("tA", "z"), ("tA", "x"), ("tC", "x")], seed=2)
    f1 = _rows([("tA", "x"), ("tB", "x"), ("tB", "y"), ("tB", "w"), ("tD", "x")], seed=3)
    f2 = _rows([("tB", "y"), ("tA", "x")], seed=4)
    pairs = C.pairs_of([f0, f1, f2])
    assert [(p.file1, p.file2, p.track, p.annotation) for p in pairs] == [
        (0, 1, "tA", "x"), (0, 1, "tB", "x"), (0, 1, "tB", "y"), (0, 2, "tA", "x"), (0, 2, "tB", "y"), (1, 2, "tA", "x"), (1, 2, "tB", "y")]
    assert pairs[1].data1 is f0[1] and pairs[1].data2 is f1[1]
    res = C.compare([f0, f1, f2], pseudo_count=0.5)
    assert [(r.track, r.annotation) for r in res] == [(p.track, p.annotation) for p in pairs]
    assert C.compare([f0, _rows([("tZ", "x")])]) == []                  # no shared track


def test_multiple_segment_tracks_in_one_file():
    with pytest.raises(NotImplementedError, match="multiple segments of interest"):
        C.compare([_rows([("tA", "x"), ("tB", "x")])])
    with pytest.raises(NotImplementedError):
        C.compare([[]])                                                   # (no track at all: the reference's test is `!= 1`)


def test_ragged_file_is_a_value_error():
    rows = _rows(["a", "b"], track="m") + _rows(["c"], n_samples=21, track="m")
    with pytest.raises(ValueError, match="20 / 21"):
        C.compare([rows])
    with pytest.raises(ValueError):
        C.compare([_rows([("t", "a")]), rows])


def test_result_fields_and_lazy_samples_of_a_result_built_from_statistics():
    """what compare() builds from the device's eight numbers: no row on the host until .samples is read"""
    d1, d2 = _rows(["a", "b"], n_samples=40, track="m")
    want = C.numpy_result(C.Pair(0, 0, d1, d2, "a", "b"), 1.0)
    s = want.samples
    st = (np.mean(s), np.std(s), want.lower95, want.upper95, np.count_nonzero(s < want.observed), np.count_nonzero(s == want.observed))
    got = gat_amd.AnnotatorResult("a", "b", "na", want.observed, C._LazyRow(d1, d2, 1.0), reference=None, pseudo_count=0, _stats=st)
    assert got._samples_cache is None
    assert str(got) == str(want) and got.pvalue == want.pvalue and got.fold == want.observed / want.expected
    assert np.array_equal(got.samples, s) and got.nsamples == 40


def test_device_threshold(monkeypatch):
    monkeypatch.delenv("GAT_DEVICE_STATS", raising=False)
    assert not C._device_wanted(C.DEVICE_MIN_VALUES - 1)
    assert C._device_wanted(C.DEVICE_MIN_VALUES) == gat_amd._numpy_summation_model_holds()
    monkeypatch.setenv("GAT_DEVICE_STATS", "1")
    assert C._device_wanted(10)
    monkeypatch.setenv("GAT_DEVICE_STATS", "0")
    assert not C._device_wanted(10 ** 9)


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_numpy_path_prints_the_reference_table(name, tmp_path, monkeypatch):
    monkeypatch.delenv("GAT_DEVICE_STATS", raising=False)              # small inputs: numpy, no device
    got, want = T.run_case(T.script(), name, str(tmp_path / "out.tsv"))
    T.assert_tables_match(got, want)
    assert got == want                                                  # (the same numpy operations: the same text)


def test_golden_set_is_what_the_issue_asks_for():
    cases = T.cases()
    assert len(cases) == 4
    a, b, single = (gat_amd.fromCounts(os.path.join(T.GOLDEN, f)) for f in ("a.counts.tsv", "b.counts.tsv", "single.counts.tsv"))
    for f in (a, b):
        assert len(set(x.track for x in f)) == 3 and len(set(x.annotation for x in f)) == 4 and len(f) == 12
        assert set(x.nsamples for x in f) == {50}
    assert len(set(x.track for x in a) & set(x.track for x in b)) == 2
    assert len(set(x.annotation for x in a) & set(x.annotation for x in b)) == 3
    assert len(set(x.track for x in single)) == 1 and len(single) == 5
    # no sample within rounding of the observed value without being equal to it (the generator asserts the same)
    for files, pc in (([a, b], 1.0), ([single], 1.0), ([single], 0.5)):
        for p in C.pairs_of(files):
            r = (p.data1.observed / (p.data1.samples + pc) + 0.0001) / (p.data2.observed / (p.data2.samples + pc) + 0.0001)
            assert np.all((np.abs(np.log(r)) > 1e-9) | (r == 1))


def test_no_results_is_logged_and_exits_0(tmp_path):
    f = tmp_path / "one.counts.tsv"
    f.write_text("track\tannotation\tobserved\tcounts\nm\ta\t10\t1,2,3\n")
    out = tmp_path / "out.txt"
    assert T.script().main(["gat-compare.py", "--stdout=%s" % out, str(f)]) == 0       # one annotation: no pair
    text = out.read_text()
    assert "no results found" in text and "track\tannotation" not in text
    assert T.script().main(["gat-compare.py", "--stdout=%s" % out]) == 0               # no file at all


_CTYPES = {"gat_ctx*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p,
           "const double*": ctypes.c_void_p, "double*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def test_ctypes_signature_matches_header():
    text = open(HEADER).read()
    m = re.search(r"\nint gat_compare_stats\((.*?)\);", text, flags=re.S)
    assert m, "gat_compare_stats is not declared"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    types = [p.rsplit(" ", 1)[0] for p in params]
    names = [p.rsplit(" ", 1)[1] for p in params]
    assert names == ["ctx", "a_dev", "n_rows_a", "b_dev", "n_rows_b", "n_samples", "ia_host", "ib_host", "n_pairs", "obs_a_host",
                     "obs_b_host", "delta_host", "pseudo_count", "lo_index", "hi_index", "out_host"]
    assert [_CTYPES[t] for t in types] == list(_lib.COMPARE_STATS_ARGTYPES)
    assert "gat_compare_stats" in _lib.SYMBOLS
    assert text.index("int gat_null_stats(") < m.start() < text.index("gat_comm_unique_id(")      # beside gat_null_stats
    knobs = open(os.path.join(ROOT, "gat_amd", "csrc", "gat_knobs.h")).read()
    assert 'REAL(compare_scratch_mb, "GAT_COMPARE_SCRATCH_MB", 1024.0)' in knobs and "GAT_COMPARE_SCRATCH_MB" in m.string
