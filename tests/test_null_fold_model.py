"""CPU: the deep null's host side (gat_amd.run(null_round_size=...), gat-run.py --null-round-size) against the Python-int
models of tests/null_fold_model.py -- a row made from its words equals AnnotatorResult's row made from the samples, words of
rounds add up to the words of the row, and every refusal is raised with its text before a device is asked for."""
import importlib.util
import os

import numpy as np
import pytest

import gat_amd
import null_fold_model as M
from gat_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Ref(object):
    def __init__(self, fold):
        self.fold = fold


def _rows(seed):
    """random integer rows: wide and narrow ranges, heavy ties, constant rows, one sample"""
    rs = np.random.RandomState(seed)
    out = []
    for n in (1, 2, 7, 100, 1000, 8192 + 331):
        out.append(rs.randint(0, 5, n))
        out.append(rs.randint(0, 1 << 40, n))
        out.append(rs.randint(1000, 1100, n))
        out.append(np.full(n, 17))
        out.append(np.zeros(n, dtype=np.int64))
    return out


def _observed(row, rs):
    lo, hi = int(row.min()), int(row.max())
    return [float(lo - 1), float(hi + 1), float(row[int(rs.randint(len(row)))]), float(np.median(row)), lo + 0.5, 0.0]


def test_a_row_from_its_words_is_the_row_from_its_samples():
    rs = np.random.RandomState(11)
    n_checked = 0
    for samples in _rows(2026):
        for observed in _observed(samples, rs):
            for fold in (None, 0.5, 3.0):
                ref = _Ref(fold) if fold is not None else None
                want = engine.AnnotatorResult("t", "a", "c", observed, samples.astype(np.float64), reference=ref)
                val = observed if fold is None else observed / fold
                w = M.row_words(samples.tolist(), val)
                model = M.row(w, observed, fold)
                assert w[1] < (1 << 53)                                   # (where numpy.mean is the exact quotient)
                assert model["nsamples"] == want.nsamples
                assert model["expected"] == want.expected, (len(samples), observed, fold)
                assert model["pvalue"] == want.pvalue, (len(samples), observed, fold)
                assert model["fold"] == want.fold
                # numpy.std sums pairwise: a few ulp times log n; 1e-12 is three orders above that, nine below anything printed
                assert abs(model["stddev"] - want.stddev) <= 1e-12 * max(want.stddev, 1e-300) or model["stddev"] == want.stddev, \
                    (model["stddev"], want.stddev)
                # the engine's own row from the same words
                raw = engine.AnnotatorResult("t", "a", "c", observed, samples.astype(np.float64))     # (the interval before the fold)
                got = engine.AnnotatorResult("t", "a", "c", observed, None, reference=ref, _words=(w, raw.lower95, raw.upper95))
                assert got.null_words == w and got.nsamples == w[0]
                assert (got.expected, got.stddev, got.pvalue, got.fold) == (model["expected"], model["stddev"], model["pvalue"], model["fold"])
                assert (got.lower95, got.upper95) == (want.lower95, want.upper95)
                assert str(got).split("\t")[:6] == str(want).split("\t")[:6] and str(got).split("\t")[7:] == str(want).split("\t")[7:]
                n_checked += 1
    assert n_checked > 500


def test_statistics_function_is_the_model():
    w = M.row_words([3, 1, 4, 1, 5, 9, 2, 6], 4.0)
    n, mean, std = engine.nullWordsStatistics(w)
    assert (n, mean, std) == (8, 31 / 8, M.row(w, 4.0)["stddev"])
    big = M.row_words([(1 << 62) + 5, (1 << 62) - 7, 3], 0.0)             # sumsq beyond 64 bits
    assert big[3] > 0 and engine.nullWordsStatistics(big)[2] == M.row(big, 0.0)["stddev"]
    with pytest.raises(ValueError, match="no samples"):
        engine.nullWordsStatistics(M.EMPTY)


def test_a_row_without_samples_says_so():
    w = M.row_words([3, 1, 4, 1, 5], 4.0)
    r = engine.AnnotatorResult("t", "a", "c", 4.0, None, _words=(w, 1.0, 5.0))
    for ask in (lambda: r.samples, lambda: r.getSample(0), lambda: r.getEmpiricalPValue(2.0)):
        with pytest.raises(ValueError, match="null_round_size / --null-round-size.*5 samples were never kept"):
            ask()
    assert r.getEmpiricalPValue(4.0) == r.pvalue                              # the value the words were counted for
    with pytest.raises(ValueError, match="never kept"):
        engine.updateQValues([r, r], method="minp")
    plain = engine.AnnotatorResult("t", "a", "c", 4.0, [3.0, 1.0, 4.0, 1.0, 5.0])
    assert plain.null_words is None and plain.pvalue == r.pvalue and plain.expected == r.expected


@pytest.mark.parametrize("size", [1, 7, "n", "beyond"])
def test_words_of_rounds_add_up(size):
    rs = np.random.RandomState(5)
    for n in (1, 6, 7, 8, 50, 257):
        values = ([int(v) for v in rs.randint(0, 1 << 62, n)] if n % 2 else [int(v) for v in rs.randint(0, 9, n)]) + [(1 << 63) - 1] * (n > 7)
        for val in (-1.0, 0.0, 4.0, 4.5, float(values[0]), 1e30):
            whole = M.row_words(values, val)
            R = {"n": len(values), "beyond": len(values) + 3}.get(size, size)
            total = M.EMPTY
            n_rounds = 0
            for b in range(0, len(values), R):
                total = M.add(total, M.row_words(values[b:b + R], val))
                n_rounds += 1
            assert total == whole, (n, val, R)
            assert n_rounds == -(-len(values) // R)


def test_the_numpy_model_is_the_python_model():
    """what the GPU tests hold the large matrices against: every limb, the clamps and the non-integer values"""
    rs = np.random.RandomState(9)
    edge = np.array([0, 1, 0xFFFF, 0x10000, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 62) - 1, 1 << 62, (1 << 63) - 1], dtype=np.uint64)
    m = np.concatenate([edge[rs.randint(0, len(edge), (6, 40))], rs.randint(0, 1 << 62, (6, 40)).astype(np.uint64),
                        rs.randint(0, 7, (6, 40)).astype(np.uint64), np.zeros((1, 40), dtype=np.uint64)])
    vals = [-3.0, 0.0, -0.0, 0.5, 3.0, 3.5, float(1 << 32), float(1 << 62), float(1 << 63), 1e30, -1e30, 4294967295.0,
            float(m[12, 0]), 6.0, 2.0 ** 63 - 1024, 1.0, 5e-324, 0.0, 2.0]
    assert len(vals) == len(m)
    assert M.words_numpy(m, vals) == M.words([[int(v) for v in row] for row in m.tolist()], vals)
    assert M.integer_parameters(1e30) == (1 << 63, None) and M.integer_parameters(-0.0) == (0, 0)
    assert M.integer_parameters(4.5) == (5, None) and M.integer_parameters(-4.0) == (0, None)


# ------------------------------------------------------------------------------------------------
# refusals: raised while the options are checked -- this machine may have no device at all, and none is asked for

def _tiny():
    segments, annotations = gat_amd.IntervalCollection("segments"), gat_amd.IntervalCollection("annotations")
    segments.add("merged", "chr1", gat_amd.SegmentList(iter=[(10, 20), (40, 45)], normalize=True))
    annotations.add("a", "chr1", gat_amd.SegmentList(iter=[(0, 30)], normalize=True))
    workspace = gat_amd.IntervalDictionary()
    workspace.add("chr1", gat_amd.SegmentList(iter=[(0, 100)], normalize=True))
    return segments, annotations, workspace


def _no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(engine, "get_context", refuse)
    monkeypatch.setattr(gat_amd, "get_context", refuse)
    monkeypatch.setattr(engine._lib, "Context", refuse)


RUN_REFUSALS = [
    (dict(output_counts_pattern="/nowhere/counts_%s"), NotImplementedError, "--output-counts-pattern has no counts to write"),
    (dict(output_samples_pattern="/nowhere/samples_%s"), NotImplementedError, "--output-samples-pattern has no sampled lists"),
    (dict(outfiles={"sample_metrics": None}), NotImplementedError, "--output-stats=sample_metrics is not written"),
    (dict(qvalue_method="minp"), NotImplementedError, "--qvalue-method=minp needs rows that hold their samples"),
    (dict(qvalue_method="efdr"), NotImplementedError, "--qvalue-method=efdr needs rows that hold their samples"),
    (dict(reference_stream=True), NotImplementedError, "per-unit streams only, not --reference-stream"),
    (dict(null_round_size=-1), ValueError, "cannot be negative"),
    (dict(null_round_size=2.5), ValueError, "an integer number of samples per round"),
]


@pytest.mark.parametrize("kwargs,error,text", RUN_REFUSALS, ids=[str(sorted(k[0].items())[0][0]) + str(i) for i, k in enumerate(RUN_REFUSALS)])
def test_run_refuses_before_a_context_is_made(kwargs, error, text, monkeypatch):
    _no_context(monkeypatch)
    segments, annotations, workspace = _tiny()
    kw = dict(num_samples=10, random_seed=1, null_round_size=4)
    kw.update(kwargs)
    with pytest.raises(error, match=text):
        gat_amd.run(segments, annotations, workspace, gat_amd.SamplerAnnotator(), [gat_amd.CounterNucleotideOverlap()],
                    gat_amd.UnconditionalWorkspace(), **kw)


def test_run_refuses_the_rest_before_a_context_is_made(monkeypatch):
    _no_context(monkeypatch)
    segments, annotations, workspace = _tiny()
    args = (segments, annotations, workspace, gat_amd.SamplerAnnotator())
    with pytest.raises(NotImplementedError, match="nucleotide-density has float rows.*nucleotide-overlap gives the same p-values"):
        gat_amd.run(*args, [gat_amd.CounterNucleotideOverlap(), gat_amd.CounterNucleotideDensity()], gat_amd.UnconditionalWorkspace(),
                    num_samples=10, null_round_size=4)
    for generator in (gat_amd.ConditionalWorkspaceCooccurance(), gat_amd.ConditionalWorkspaceAnnotationCentered(None, 2.0),
                      gat_amd.ConditionalWorkspaceSegmentCentered(None, 2.0)):
        with pytest.raises(NotImplementedError, match="only --conditional=unconditional"):
            gat_amd.run(*args, [gat_amd.CounterNucleotideOverlap()], generator, num_samples=10, null_round_size=4)
    monkeypatch.setattr(gat_amd, "_dist_state", lambda: (0, 2, "gloo"))
    with pytest.raises(NotImplementedError, match="not sharded over the 2 ranks"):
        gat_amd.run(*args, [gat_amd.CounterNucleotideOverlap()], gat_amd.UnconditionalWorkspace(), num_samples=10, null_round_size=4)


def test_the_default_refuses_nothing():
    gat_amd.check_null_round_options(0, counters=["nucleotide-density"], conditional="cooccurance", reference_stream=True,
                                     output_counts_pattern="c%s", output_samples_pattern="s%s",
                                     output_stats=["sample_metrics", "fdr_summary"], qvalue_method="minp")
    gat_amd.check_null_round_options(5, counters=[n for n in gat_amd.COUNTERS if n != "nucleotide-density"], qvalue_method="BH",
                                     output_stats=["segment_metrics", "all"])


def test_units_refusals():
    gat_amd._check_null_round_units(1 << 20, 1 << 12, 3_000_000_000)              # exactly 2^32 streams: each used once
    with pytest.raises(ValueError, match=r"more than the 2\^32 unit streams.*this problem allows 1048320 samples"):
        gat_amd._check_null_round_units((1 << 20) + 1, (1 << 12) + 1, 3_000_000_000)
    with pytest.raises(ValueError, match=r"this problem allows 178956970 samples"):
        gat_amd._check_null_round_units(10 ** 9, 24, 3_000_000_000)
    with pytest.raises(ValueError, match="no longer fits its 64-bit word"):
        gat_amd._check_null_round_units(1 << 31, 1, 1 << 32)
    gat_amd._check_null_round_units((1 << 31) - 1, 1, 1 << 32)


CLI_REFUSALS = [
    (["--output-counts-pattern=/nowhere/c_%s"], "--output-counts-pattern has no counts to write"),
    (["--output-samples-pattern=/nowhere/s_%s"], "--output-samples-pattern has no sampled lists"),
    (["--output-stats=sample_metrics"], "--output-stats=sample_metrics is not written"),
    (["--output-stats=fdr_summary"], "--output-stats=fdr_summary needs rows that hold their samples"),
    (["--qvalue-method=minp"], "--qvalue-method=minp needs rows"),
    (["--qvalue-method=efdr"], "--qvalue-method=efdr needs rows"),
    (["--conditional=cooccurance"], r"only --conditional=unconditional \(got cooccurance"),
    (["--conditional=segment-centered", "--conditional-expansion=2"], r"only --conditional=unconditional \(got segment-centered"),
    (["--reference-stream"], "not --reference-stream"),
    (["--counter=nucleotide-overlap", "--counter=nucleotide-density"], "nucleotide-density has float rows"),
]


@pytest.mark.parametrize("extra,text", CLI_REFUSALS, ids=[e[0][0].lstrip("-") for e in CLI_REFUSALS])
def test_cli_refuses_before_a_file_is_read(extra, text, tmp_path, monkeypatch):
    """the input files do not exist: the refusal comes before anything looks for them"""
    _no_context(monkeypatch)
    spec = importlib.util.spec_from_file_location("gat_run_deep", os.path.join(ROOT, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = ["gat-run.py", "--segments=/nowhere/s.bed", "--annotations=/nowhere/a.bed", "--workspace=/nowhere/w.bed",
            "--num-samples=100", "--null-round-size=32", "--stdout=%s" % str(tmp_path / "out.tsv"), "--log=%s" % str(tmp_path / "log")] + extra
    with pytest.raises(NotImplementedError, match=text):
        mod.main(argv)
    with pytest.raises(ValueError, match="cannot be negative"):
        mod.main(argv[:5] + ["--null-round-size=-3"] + argv[6:])


def test_the_option_says_whose_interval_it_prints():
    parser = gat_amd.buildParser()
    opt = parser.get_option("--null-round-size")
    assert opt.type == "int" and parser.get_default_values().null_round_size == 0
    assert "CI95low and CI95high" in opt.help and "FIRST round" in opt.help
