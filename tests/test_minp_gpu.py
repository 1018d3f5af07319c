"""GPU: gat_minp_counts (k_minp_rank + k_minp_step) against the numpy model of tests/minp_model.py: the counts c are
integers and are compared for equality, row by row, none skipped -- over the wave and workgroup edges of S, both sort paths
(GAT_MINP_LDS_SAMPLES at its default and at 64), one batch and several (GAT_MINP_SCRATCH_MB at its default and at two rows
of K: the carried q), a seeded fuzz loop, the error returns, and scripts/gat-run.py --qvalue-method=minp end to end."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import gat_amd
import minp_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _slots(m, is_double):
    """the matrix as gat_null_stats' layout holds it: 8-byte slots, int64, or the double's bits for the flagged rows"""
    out = np.zeros(m.shape, dtype=np.int64)
    for r in range(m.shape[0]):
        if is_double[r]:
            out[r] = m[r].view(np.int64)
        else:
            assert np.array_equal(m[r], np.round(m[r]))
            out[r] = m[r].astype(np.int64)
    return out


def _device_counts(ctx, m, is_double, means, k_obs):
    slots = _slots(m, is_double)
    ptr = ctx.alloc(slots.nbytes)
    try:
        ctx.h2d(ptr, slots)
        return ctx.minp_counts(ptr, m.shape[0], m.shape[1], is_double, means, k_obs).tolist()
    finally:
        ctx.free(ptr)


_MODEL = {}


def _family(R, S, first):
    """a shape's family and the model's answer for it, computed once and shared by the knob settings"""
    key = (R, S, first)
    if key not in _MODEL:
        m, is_double, obs = M.family(np.random.RandomState(7919 * R + 31 * S + first), R, S, first)
        means = [float(np.mean(row)) for row in m]
        k_obs, c, _ = M.minp(m, means, obs)
        for a in (m, is_double):
            a.setflags(write=False)
        _MODEL[key] = (m, is_double, means, k_obs, c)
    return _MODEL[key]


def _two_rows_mb(S):
    return repr(2 * S * 4 / 1048576.0)


@pytest.mark.parametrize("scratch", ["default", "two rows"])
@pytest.mark.parametrize("lds", ["default", "64"])
@pytest.mark.parametrize("R", [1, 2, 7, 40])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_counts_equal_the_model(ctx, S, R, lds, scratch, monkeypatch):
    if lds != "default":
        monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", lds)          # S = 65 .. 1000: the global-memory sort
    if scratch != "default":
        monkeypatch.setitem(ctx.options, "GAT_MINP_SCRATCH_MB", _two_rows_mb(S))   # R = 7, 40: several batches, q carried
    for first in (range(0, M.N_KINDS, R) if R < M.N_KINDS else [0]):
        m, is_double, means, k_obs, want = _family(R, S, first)
        got = _device_counts(ctx, m, is_double, means, k_obs)
        print("S=%d R=%d first=%d lds=%s scratch=%s: k_obs=%s c=%s" % (S, R, first, lds, scratch, k_obs[:8], got[:8]))
        assert got == want


def test_every_kind_of_row_is_in_the_families():
    """what the shapes above rest on: the ties, both constant rows, the double row, the tie in the order, and observed values
    below, inside and above the sampled range"""
    m, is_double, means, k_obs, c = _family(40, 1000, 0)
    S = 1000
    assert len(np.unique(m[0])) == 3 and k_obs[1] == S and k_obs[2] == 1
    assert is_double[3] == 1 and m[3].min() < 0 and np.any((np.abs(m[3]) < 1) & (m[3] != 0))
    assert k_obs[4] == k_obs[5] and M.order(k_obs).index(4) + 1 == M.order(k_obs).index(5)
    obs = M.family(np.random.RandomState(7919 * 40 + 31 * S), 40, S, 0)[2]
    assert any(o < row.min() for o, row in zip(obs, m)) and any(o > row.max() for o, row in zip(obs, m))
    assert any(row.min() < o < row.max() for o, row in zip(obs, m))
    m1, _, _, k1, c1 = _family(1, 65, 2)
    assert k1 == [1] and c1 == [0]                                            # the constant row, observed off it, alone


def test_all_digit_passes_give_the_same_counts(ctx, monkeypatch):
    m, is_double, means, k_obs, want = _family(7, 257, 0)
    for lds in ("4096", "64"):
        monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", lds)
        monkeypatch.setitem(ctx.options, "GAT_MINP_ALL_PASSES", "1")
        assert _device_counts(ctx, m, is_double, means, k_obs) == want


def test_fuzz(ctx, monkeypatch):
    """a few hundred small families under a fixed seed: ties, doubles, random knobs; every count equal"""
    rs = np.random.RandomState(424242)
    n = 0
    for it in range(300):
        R, S = int(rs.randint(1, 13)), int(rs.randint(1, 301))
        m = np.zeros((R, S))
        is_double = (rs.uniform(size=R) < 0.3).astype(np.uint8)
        for r in range(R):
            if is_double[r]:
                m[r] = np.round(rs.normal(0, 2, S), int(rs.randint(0, 3)))
            else:
                lo = int(rs.randint(0, 1000))
                m[r] = rs.randint(lo, lo + int(rs.choice([1, 2, 5, 50, 100000])), S)
            if rs.uniform() < 0.2 and r > 0:
                m[r] = m[r - 1]
                is_double[r] = is_double[r - 1]
        obs = np.array([rs.choice([row.min() - 1, row.max() + 1, row[0], float(np.median(row))]) for row in m])
        means = [float(np.mean(row)) for row in m]
        k_obs, want, _ = M.minp(m, means, obs)
        monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", str(rs.choice([0, 64, 128, 4096])))
        monkeypatch.setitem(ctx.options, "GAT_MINP_SCRATCH_MB", repr(int(rs.randint(1, R + 2)) * S * 4 / 1048576.0))
        got = _device_counts(ctx, m, is_double, means, k_obs)
        assert got == want, (it, R, S)
        n += R
    assert n > 1000


def test_adjust_on_the_device_equals_the_model(ctx):
    from gat_amd import minp
    m, _, means, k_obs, c = _family(40, 1000, 0)
    obs = M.family(np.random.RandomState(7919 * 40 + 31 * 1000), 40, 1000, 0)[2]
    rows = [gat_amd.AnnotatorResult("t", "a%d" % i, "na", o, row) for i, (row, o) in enumerate(zip(m, obs))]
    assert [r.expected for r in rows] == means
    assert minp.adjust(rows, ctx=ctx) == M.adjusted(k_obs, c, 1000)


def test_error_returns(ctx, monkeypatch):
    L = _lib.lib()
    GAT_ERR_ARG = -6
    R, S = 3, 10
    slots = np.arange(R * S, dtype=np.int64).reshape(R, S)
    ptr = ctx.alloc(slots.nbytes)
    try:
        ctx.h2d(ptr, slots)
        dbl = np.zeros(R, dtype=np.uint8)
        means = slots.mean(axis=1)
        kobs = np.array([1, 5, 10], dtype=np.int32)
        out = np.full(R, -7, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        dev = ctypes.c_void_p(ptr)

        def call(h=ctx._h, d=dev, nr=R, ns=S, a=dbl, b=means, k=kobs, o=out):
            return L.gat_minp_counts(h, d, nr, ns, None if a is None else p(a), None if b is None else p(b),
                                     None if k is None else p(k), None if o is None else p(o))
        assert call() == 0 and out.tolist() == M.counts(slots.astype(np.float64), means.tolist(), kobs.tolist())
        for kw in (dict(h=None), dict(d=None), dict(a=None), dict(b=None), dict(k=None), dict(o=None)):
            assert call(**kw) == GAT_ERR_ARG, kw
        assert call(ns=0) == GAT_ERR_ARG and call(ns=-1) == GAT_ERR_ARG and call(ns=2 ** 31) == GAT_ERR_ARG
        for bad in (0, -1, S + 1):
            assert call(k=np.array([1, bad, 10], dtype=np.int32)) == GAT_ERR_ARG, bad
        out[:] = -7
        assert call(nr=0) == 0 and call(nr=-3) == 0 and out.tolist() == [-7] * R      # nothing to do, nothing written
        for mb in ("0", "-1"):
            monkeypatch.setitem(ctx.options, "GAT_MINP_SCRATCH_MB", mb)
            assert call() == GAT_ERR_ARG, mb
        monkeypatch.delitem(ctx.options, "GAT_MINP_SCRATCH_MB")
        for n in ("-1", "1000000"):                                                  # more than a workgroup's LDS holds
            monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", n)
            assert call() == GAT_ERR_ARG, n
        monkeypatch.delitem(ctx.options, "GAT_MINP_LDS_SAMPLES")
        assert call() == 0
        with pytest.raises(ValueError):
            ctx.minp_counts(ptr, R, S, dbl, means, [1, 11, 10])
    finally:
        ctx.free(ptr)


def _run_cli(tmp_path, tag, extra):
    spec = importlib.util.spec_from_file_location("gat_run_minp", os.path.join(ROOT, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / ("%s.tsv" % tag))
    argv = ["gat-run.py", "--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=100", "--random-seed=5",
            "--stdout=%s" % out, "--log=%s" % str(tmp_path / ("%s.log" % tag))] + extra
    assert mod.main(argv) == 0
    return [line for line in open(out) if not line.startswith("#")]


def test_cli_minp_end_to_end(tmp_path):
    """gat-run.py --qvalue-method=minp on the golden command-line inputs: the first ten columns are the golden table's, the
    qvalue column is the model applied to the run's own counts file; --qvalue-method=BH still prints the golden table"""
    want = [line for line in open(os.path.join(CLI, "expected_default.tsv")) if not line.startswith("#")]
    pattern = str(tmp_path / "counts_%s.tsv")
    got = _run_cli(tmp_path, "minp", ["--qvalue-method=minp", "--output-counts-pattern=%s" % pattern])
    assert len(got) == len(want) > 2
    assert [line.split("\t")[:10] for line in got] == [line.split("\t")[:10] for line in want]
    assert [line.split("\t")[11:] for line in got] == [line.split("\t")[11:] for line in want]
    rows = gat_amd.fromCounts(pattern % "nucleotide-overlap")
    m = np.stack([r.samples for r in rows])
    _, _, adj = M.minp(m, [float(np.mean(row)) for row in m], [r.observed for r in rows])
    model = dict(((r.track, r.annotation), "%6.4e" % q) for r, q in zip(rows, adj))
    assert len(model) == len(got) - 1
    for line in got[1:]:
        f = line.split("\t")
        assert f[10] == model[(f[0], f[1])], line
    assert any(line.split("\t")[10] != w.split("\t")[10] for line, w in zip(got[1:], want[1:])) or len(got) <= 2
    assert _run_cli(tmp_path, "bh", ["--qvalue-method=BH"]) == want
