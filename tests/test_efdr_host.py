"""CPU: the host side of --qvalue-method=efdr / --output-stats=fdr_summary (gat_amd/efdr.py, the parser, IO.outputResults,
engine.updateQValues) -- what needs no device: q-values and summary statistics from given integer arrays against the model of
tests/efdr_model.py, the command line's options, and the ValueErrors, which are raised before a context is touched."""
import importlib.util
import io
import os
import types

import numpy as np
import pytest

import efdr_model as E
import gat_amd
import minp_model as M
from gat_amd import IO, efdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name.replace("-", "_") + "_efdr_host", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model_family(R, S, seed, first=0):
    m, _, obs = M.family(np.random.RandomState(seed), R, S, first)
    means = [float(np.mean(row)) for row in m]
    k_obs = M.k_obs_of(m, means, obs)
    return m, means, obs, k_obs


@pytest.mark.parametrize("R,S", [(1, 1), (3, 1), (2, 2), (7, 65), (40, 257)])
def test_adjusted_equals_the_model(R, S):
    for first in (range(0, M.N_KINDS, R) if R < M.N_KINDS else [0]):
        m, means, obs, k_obs = _model_family(R, S, 31 * R + S + first, first)
        v = E.counts(m, means, k_obs)
        got = efdr.adjusted(k_obs, np.array(v, dtype=np.int64), S)
        assert got == E.adjusted(k_obs, v, S)
        assert all(isinstance(x, float) for x in got)


def test_adjusted_ties_in_kobs_share_rn():
    # rows 0, 1 and 3 are tied at k_obs 3: Rn = 3 for each of them, 4 at k_obs 10
    k_obs = [3, 3, 10, 3]
    v = [[4, 2], [4, 2], [8, 4], [4, 2]]
    assert efdr.adjusted(k_obs, v, 10) == E.adjusted(k_obs, v, 10) == [0.2, 0.2, 0.3, 0.2]
    assert efdr.adjusted([1], [[0, 0]], 4) == [0.25]                          # the floor 1 / S
    assert efdr.adjusted([1, 1], [[9, 9], [9, 9]], 1) == [1.0, 1.0]           # the cap
    assert efdr.adjusted([], [], 10) == []


@pytest.mark.parametrize("R,S", [(3, 1), (7, 65), (40, 257)])
def test_summary_statistics_equal_the_model(R, S):
    m, means, obs, k_obs = _model_family(R, S, 77 * R + S)
    cutoffs = [0.0, 0.001, 0.05, 0.2, 1.0]                                    # S = 65, 257: 0.001 * S < 1 -> level 0 -> na
    levels = [int(p * S) for p in cutoffs]
    per = E.per_sample(m, means, levels)
    d_obs = [o > e for o, e in zip(obs, means)]
    rows = efdr.summarise(k_obs, d_obs, per.astype(np.int32), cutoffs, S)
    want = E.summary(m, means, obs, cutoffs)
    assert rows == want
    assert efdr.format_summary(rows) == E.format_summary(want)
    assert [r[4:] for r in rows[:3]] == [("na", "na", "na")] * 3
    assert efdr.format_summary(rows).splitlines()[0] == "pvalue_cutoff\tlevel\tcategory\tobserved\taverage\tmedian\tlimit95"
    assert [r[2] for r in rows[:3]] == ["significant", "over", "under"]


def test_both_parsers_take_the_options():
    for parser in (gat_amd.buildParser(samplers=gat_amd.CLI_SAMPLERS), _script("gat-distance").buildParser()):
        o, _ = parser.parse_args([])
        assert o.qvalue_method == "BH" and not o.fdr_summary_pvalues and o.output_stats == []
        o, _ = parser.parse_args(["--qvalue-method=efdr", "--output-stats=fdr_summary", "--fdr-summary-pvalue=0.05",
                                  "--fdr-summary-pvalue=0.2"])
        assert o.qvalue_method == "efdr" and o.output_stats == ["fdr_summary"] and o.fdr_summary_pvalues == [0.05, 0.2]
    assert _script("gat-run").main is not None
    o, _ = gat_amd.buildParser().parse_args([])
    assert o.qvalue_method == "BH"
    with pytest.raises(SystemExit):
        gat_amd.buildParser().parse_args(["--qvalue-method=efdr2"])


def _options(**kw):
    o = types.SimpleNamespace(qvalue_method="efdr", pvalue_method="empirical", output_stats=[], output_order="fold",
                              output_tables_pattern="%s.tsv", stdout=io.StringIO(), fdr_summary_pvalues=None,
                              output_filename_pattern="%s", output_force=False)
    o.__dict__.update(kw)
    return o


def _row(n=10, annotation="a", **kw):
    return gat_amd.AnnotatorResult("t", annotation, "na", 3.0, np.arange(n, dtype=np.float64), **kw)


def test_value_errors_come_before_the_device(tmp_path, monkeypatch):
    import gat_amd.engine as engine

    def no_device(*a, **k):
        raise AssertionError("the context was asked for")
    monkeypatch.setattr(engine, "get_context", no_device)
    header = gat_amd.AnnotatorResult.headers
    with pytest.raises(ValueError, match="--qvalue-method=efdr needs --pvalue-method=empirical"):
        IO.outputResults([_row()], _options(pvalue_method="norm"), header)
    with pytest.raises(ValueError, match="--output-stats=fdr_summary needs --pvalue-method=empirical"):
        IO.outputResults([_row()], _options(qvalue_method="BH", pvalue_method="norm", output_stats=["fdr_summary"]), header)
    read_back = IO.DummyAnnotatorResult._fromLine("t\ta\t3\t1.0\t0.5\t1.5\t0.2\t3.0\t1.58\t1e-3\t1e-2\n")
    fold = types.SimpleNamespace(fold=2.0)
    for rows, text in (([_row(), read_back], "holds no samples"),
                       ([_row(), _row(annotation="b", reference=fold)], "was built with a reference"),
                       ([_row(10), _row(11, annotation="b")], "rows of 10 and 11 samples")):
        for call in (lambda: efdr.adjust(rows), lambda: efdr.summary(rows, [0.05]), lambda: efdr.compute(rows, [0.05]),
                     lambda: gat_amd.engine.updateQValues(rows, method="efdr"),
                     lambda: IO.outputResults(rows, _options(), header),
                     lambda: IO.outputResults(rows, _options(qvalue_method="BH", output_stats=["fdr_summary"],
                                                             output_filename_pattern=str(tmp_path / "%s.tsv")), header)):
            with pytest.raises(ValueError, match="qvalue method efdr.*" + text):
                call()
    assert not os.path.exists(str(tmp_path / "fdr_summary.tsv"))
    assert efdr.compute([], [0.05]) == ([], [])
