"""CPU: the numpy model of step-down minP (tests/minp_model.py) against the project's own p-value, its invariants, and the
host half of gat_amd.minp -- ordering, running maximum, the three ValueErrors -- with a stub in place of the device call."""
import numpy as np
import pytest

import gat_amd
import minp_model as M
from gat_amd import engine


def _families():
    rs = np.random.RandomState(20260)
    for R, S in [(1, 1), (1, 2), (2, 3), (3, 17), (7, 64), (7, 65), (12, 200), (40, 1000)]:
        for first in range(0, M.N_KINDS, R) if R < M.N_KINDS else [0]:
            m, _, obs = M.family(rs, R, S, first)
            yield m, np.array([float(np.mean(row)) for row in m]), obs


def test_t_over_s_is_the_projects_pvalue():
    """T / S == getTwoSidedPValue(sorted row, mean, x) for x = the observed value and x = every sample, and t_row (the
    vectorised form the procedure uses) == t_value sample by sample"""
    n = 0
    for m, e, obs in _families():
        S = m.shape[1]
        for row, mean, o in zip(m, e, obs):
            s = np.sort(row)
            assert float(M.t_value(row, mean, o)) / S == engine.getTwoSidedPValue(s, mean, o)
            K = M.t_row(row, mean)
            for x, k in zip(row.tolist(), K.tolist()):
                assert k == M.t_value(row, mean, x)
                assert float(k) / S == engine.getTwoSidedPValue(s, mean, x)
                n += 1
            r = gat_amd.AnnotatorResult("t", "a", "na", o, row)
            assert r.pvalue == float(M.t_value(row, mean, o)) / S and r.expected == mean
    assert n > 40000


def test_adjusted_values_dominate_the_raw_ones_and_follow_the_order():
    for m, e, obs in _families():
        S = m.shape[1]
        k_obs, c, adj = M.minp(m, e, obs)
        o = M.order(k_obs)
        assert sorted(o) == list(range(len(m))) and all((k_obs[a], a) < (k_obs[b], b) for a, b in zip(o, o[1:]))
        for r in range(len(m)):
            assert 0 <= c[r] <= S and 1.0 / S <= adj[r] <= 1.0
            assert adj[r] >= float(k_obs[r]) / S                        # never below the raw p-value
        assert all(adj[a] <= adj[b] for a, b in zip(o, o[1:]))          # non-decreasing along the order


def test_constant_rows():
    """a constant row with the observed value on the constant has k_obs = S; with it off the constant k_obs = 1, and no
    sample of the row itself reaches that (c = 0 where no other row stands behind it in the order)"""
    rs = np.random.RandomState(3)
    m, _, obs = M.family(rs, 7, 50)
    e = [float(np.mean(r)) for r in m]
    k_obs, c, adj = M.minp(m, e, obs)
    assert k_obs[1] == 50 and k_obs[2] == 1 and adj[2] == min(adj)
    assert k_obs[4] == k_obs[5]                                         # the tie the row index resolves
    m, _, obs = M.family(rs, 1, 50, first=2)
    assert M.minp(m, [12.0], obs) == ([1], [0], [1.0 / 50])


class _StubContext(object):
    """stands where the device does: minp_counts is the model's, on the matrix that was "uploaded" """

    def __init__(self):
        self.calls = []
        self.held = {}

    def alloc(self, nbytes):
        self.held[len(self.held) + 1] = None
        return len(self.held)

    def h2d(self, ptr, host_array):
        assert ptr in self.held
        self.held[ptr] = np.array(host_array, copy=True)

    def free(self, ptr):
        del self.held[ptr]

    def minp_counts(self, ptr, n_rows, n_samples, is_double, means, k_obs):
        m = self.held[ptr]
        assert m.dtype == np.float64 and m.shape == (n_rows, n_samples) and list(is_double) == [1] * n_rows
        self.calls.append((n_rows, n_samples))
        return np.array(M.counts(m, list(means), list(k_obs)), dtype=np.int64)


def _results(m, obs):
    return [gat_amd.AnnotatorResult("t", "a%d" % i, "na", o, row) for i, (row, o) in enumerate(zip(m, obs))]


def test_host_half_of_adjust_with_a_stub_device():
    from gat_amd import minp
    for m, e, obs in _families():
        stub = _StubContext()
        got = minp.adjust(_results(m, obs), ctx=stub)
        k_obs, c, want = M.minp(m, e, obs)
        assert got == want and stub.calls == [m.shape] and stub.held == {}
        assert minp.order(k_obs) == M.order(k_obs) and minp.adjusted(k_obs, c, m.shape[1]) == want
    assert minp.adjust([], ctx=_StubContext()) == []
    # the running maximum is taken along the order, not along the rows: counts that fall along the order are lifted
    assert minp.adjusted([3, 1, 2], [2, 5, 0], 10) == [0.5, 0.5, 0.5]
    assert minp.adjusted([2, 2, 1], [4, 3, 0], 10) == [0.4, 0.4, 0.1]


def test_adjust_refuses_what_the_procedure_does_not_cover():
    from gat_amd import IO, minp
    rs = np.random.RandomState(5)
    a = gat_amd.AnnotatorResult("t", "a", "na", 4.0, rs.randint(0, 9, 20))
    b = gat_amd.AnnotatorResult("t", "b", "na", 4.0, rs.randint(0, 9, 21))
    with pytest.raises(ValueError, match="samples"):
        minp.adjust([a, b], ctx=_StubContext())                          # rows of different nsamples
    line = str(a) + "\n"
    dummy = IO.DummyAnnotatorResult._fromLine(line)
    with pytest.raises(ValueError, match="holds no samples"):
        minp.adjust([a, dummy], ctx=_StubContext())                      # a table read back holds no samples
    ref = gat_amd.AnnotatorResult("t", "r", "na", 5.0, rs.randint(1, 9, 20))
    c = gat_amd.AnnotatorResult("t", "c", "na", 4.0, rs.randint(1, 9, 20), reference=ref)
    with pytest.raises(ValueError, match="reference"):
        minp.adjust([a, c], ctx=_StubContext())                          # expected is no longer the row's mean


def test_dispatch_and_command_line():
    """stats.getQValues is a function of p-values alone and does not know minp; the parsers offer it; with
    --pvalue-method=norm it is refused before anything is computed"""
    import importlib.util
    import os
    from gat_amd import IO, stats
    with pytest.raises(NotImplementedError, match="adjustment method"):
        stats.getQValues([0.1, 0.2], method="minp")
    opts, _ = gat_amd.buildParser().parse_args(["--qvalue-method=minp"])
    assert opts.qvalue_method == "minp"
    assert gat_amd.buildParser().parse_args([])[0].qvalue_method == "BH"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gat_distance_cli", os.path.join(root, "scripts", "gat-distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.buildParser().parse_args(["--qvalue-method=minp"])[0].qvalue_method == "minp"
    opts, _ = gat_amd.buildParser().parse_args(["--qvalue-method=minp", "--pvalue-method=norm"])
    rs = np.random.RandomState(6)
    rows = [gat_amd.AnnotatorResult("t", "a", "na", 4.0, rs.randint(0, 9, 20))]
    with pytest.raises(ValueError, match="pvalue-method"):
        IO.outputResults(rows, opts, gat_amd.AnnotatorResult.headers)
