"""GPU: gat_efdr_counts (k_minp_rank + k_efdr) against the numpy model of tests/efdr_model.py: V and the per-sample level counts
are integers and are compared for equality, none skipped -- over the wave and workgroup edges of S, one batch and several
(GAT_MINP_SCRATCH_MB at two rows of K: bins and per-sample counts carried), one threshold chunk and several
(GAT_EFDR_LDS_THRESHOLDS=2), both sort paths of the rank step, a seeded fuzz loop, the error returns, efdr.adjust /
efdr.summary, and the two scripts end to end."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import efdr_model as E
import gat_amd
import minp_model as M
from gat_amd import _lib, efdr

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


def _device(ctx, m, is_double, means, k_obs, levels):
    slots = _slots(m, is_double)
    ptr = ctx.alloc(slots.nbytes)
    try:
        ctx.h2d(ptr, slots)
        v, per = ctx.efdr_counts(ptr, m.shape[0], m.shape[1], is_double, means, k_obs, levels)
        return v.tolist(), per.tolist()
    finally:
        ctx.free(ptr)


def _levels(S):
    return [0, 1, int(0.05 * S), S]


_MODEL = {}


def _family(R, S, first):
    """a shape's family and the model's answer for it, computed once and shared by the knob settings"""
    key = (R, S, first)
    if key not in _MODEL:
        m, is_double, obs = M.family(np.random.RandomState(7919 * R + 31 * S + first), R, S, first)
        means = [float(np.mean(row)) for row in m]
        k_obs = M.k_obs_of(m, means, obs)
        v = E.counts(m, means, k_obs)
        per = E.per_sample(m, means, _levels(S)).tolist()
        for a in (m, is_double, obs):
            a.setflags(write=False)
        _MODEL[key] = (m, is_double, means, obs, k_obs, v, per)
    return _MODEL[key]


KNOBS = {"default": {},
         "two rows of K": None,                                              # GAT_MINP_SCRATCH_MB, by S
         "chunks of 2 thresholds": {"GAT_EFDR_LDS_THRESHOLDS": "2"},
         "sort in global memory": {"GAT_MINP_LDS_SAMPLES": "64"}}


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("R", [1, 2, 7, 40])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_counts_equal_the_model(ctx, S, R, knobs, monkeypatch):
    settings = KNOBS[knobs] if KNOBS[knobs] is not None else {"GAT_MINP_SCRATCH_MB": repr(2 * S * 4 / 1048576.0)}
    for name, value in settings.items():
        monkeypatch.setitem(ctx.options, name, value)
    for first in (range(0, M.N_KINDS, R) if R < M.N_KINDS else [0]):
        m, is_double, means, _, k_obs, want_v, want_per = _family(R, S, first)
        v, per = _device(ctx, m, is_double, means, k_obs, _levels(S))
        print("S=%d R=%d first=%d %s: k_obs=%s v=%s" % (S, R, first, knobs, k_obs[:6], v[:6]))
        assert v == want_v
        assert per == want_per


def test_every_kind_of_row_is_in_the_families():
    """what the shapes above rest on: the ties, both constant rows, the double row with -0.0, the duplicated rows, observed values
    below, inside and above the sampled range -- and several distinct thresholds, so that chunks of two are several chunks"""
    S = 1000
    m, is_double, means, obs, k_obs, v, per = _family(40, S, 0)
    assert len(np.unique(m[0])) == 3 and k_obs[1] == S and k_obs[2] == 1
    assert is_double[3] == 1 and np.any((m[3] == 0) & np.signbit(m[3]))
    assert np.array_equal(m[4], m[5]) and k_obs[4] == k_obs[5]
    assert any(o < row.min() for o, row in zip(obs, m)) and any(o > row.max() for o, row in zip(obs, m))
    assert any(row.min() < o < row.max() for o, row in zip(obs, m))
    assert len(set(k_obs)) > 6
    assert v[1] == [int(np.count_nonzero(m > np.array(means)[:, None])), int(np.count_nonzero(m <= np.array(means)[:, None]))]   # t = S: everything


def test_fuzz(ctx, monkeypatch):
    """300 small families under a fixed seed, drawn as tests/test_minp_gpu.py::test_fuzz draws them: ties, doubles, 0 to 8
    levels, random knobs; every count equal"""
    rs = np.random.RandomState(535353)
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
        levels = [int(x) for x in rs.randint(0, S + 1, int(rs.randint(0, 9)))]
        k_obs = M.k_obs_of(m, means, obs)
        monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", str(rs.choice([0, 64, 128, 4096])))
        monkeypatch.setitem(ctx.options, "GAT_MINP_SCRATCH_MB", repr(int(rs.randint(1, R + 2)) * S * 4 / 1048576.0))
        monkeypatch.setitem(ctx.options, "GAT_EFDR_LDS_THRESHOLDS", str(rs.choice([1, 2, 3, 5, 13000])))
        v, per = _device(ctx, m, is_double, means, k_obs, levels)
        assert v == E.counts(m, means, k_obs), (it, R, S)
        assert per == E.per_sample(m, means, levels).tolist(), (it, R, S, levels)
        n += R
    assert n > 1000


def test_more_thresholds_than_64_kib_of_lds(ctx):
    """5 600 distinct thresholds are 67 200 bytes of LDS: the launch needs the kernel's opt-in beyond 64 KiB, and a slab of rows is
    set by the thresholds (one row per 32).  Every row is a rotation of one permutation of 0 .. S-1, for which T has a closed
    form (n_less = the value, n_eq = 1) -- checked against the model on three rows -- so that V is a histogram and its running sum"""
    R = S = 5600
    perm = np.random.RandomState(56).permutation(S).astype(np.int64)
    slots = (perm[None, :] + 37 * np.arange(R, dtype=np.int64)[:, None]) % S
    mean = (S - 1) / 2.0
    D = slots > mean
    K = np.maximum(1, np.where(D, S - slots, slots + 1))
    means = [float(np.mean(slots[r])) for r in (0, 1, R - 1)]
    assert means == [mean] * 3
    for r in (0, 1, R - 1):
        assert np.array_equal(K[r], M.t_row(slots[r].astype(np.float64), mean))
    k_obs = np.arange(1, R + 1, dtype=np.int32)                                      # every threshold once
    L = int(0.05 * S)
    want_v = np.stack([np.cumsum(np.bincount(K[D], minlength=S + 1))[k_obs], np.cumsum(np.bincount(K[~D], minlength=S + 1))[k_obs]], axis=1)
    want_per = np.stack([np.count_nonzero((K <= L) & D, axis=0), np.count_nonzero((K <= L) & ~D, axis=0)])
    ptr = ctx.alloc(slots.nbytes)
    try:
        ctx.h2d(ptr, slots)
        v, per = ctx.efdr_counts(ptr, R, S, np.zeros(R, dtype=np.uint8), np.full(R, mean), k_obs, [L])
    finally:
        ctx.free(ptr)
    assert int(want_v[-1].sum()) == R * S
    assert np.array_equal(v, want_v)
    assert np.array_equal(per[0], want_per)


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
        levels = np.array([0, 10], dtype=np.int32)
        v = np.full((R, 2), -7, dtype=np.int64)
        per = np.full((2, 2, S), -7, dtype=np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        dev = ctypes.c_void_p(ptr)

        def call(h=ctx._h, d=dev, nr=R, ns=S, a=dbl, b=means, k=kobs, lv=levels, nl=2, o=v, ps=per):
            return L.gat_efdr_counts(h, d, nr, ns, p(a), p(b), p(k), p(lv), nl, p(o), p(ps))
        fm = slots.astype(np.float64)
        assert call() == 0
        assert v.tolist() == E.counts(fm, means.tolist(), kobs.tolist())
        assert per.tolist() == E.per_sample(fm, means.tolist(), [0, 10]).tolist() and per[0].sum() == 0 and per[1].sum() == R * S
        for kw in (dict(h=None), dict(d=None), dict(a=None), dict(b=None), dict(k=None), dict(o=None), dict(ps=None), dict(lv=None)):
            assert call(**kw) == GAT_ERR_ARG, kw
        assert call(nl=0, ps=None, lv=None) == 0                                     # no levels: nothing to write them to
        assert call(ns=0) == GAT_ERR_ARG and call(ns=-1) == GAT_ERR_ARG and call(ns=2 ** 31) == GAT_ERR_ARG
        for bad in (0, -1, S + 1):
            assert call(k=np.array([1, bad, 10], dtype=np.int32)) == GAT_ERR_ARG, bad
        assert call(nl=-1) == GAT_ERR_ARG and call(nl=9, lv=np.zeros(9, dtype=np.int32), ps=np.zeros((9, 2, S), dtype=np.int32)) == GAT_ERR_ARG
        for bad in (-1, S + 1):
            assert call(lv=np.array([0, bad], dtype=np.int32)) == GAT_ERR_ARG, bad
        v[:] = -7
        per[:] = -7
        assert call(nr=0) == 0 and call(nr=-3) == 0                                  # nothing to do, nothing written
        assert v.tolist() == [[-7, -7]] * R and np.all(per == -7)
        for name, values in (("GAT_MINP_SCRATCH_MB", ("0", "-1")), ("GAT_MINP_LDS_SAMPLES", ("-1", "1000000")),
                             ("GAT_EFDR_LDS_THRESHOLDS", ("0", "-1", "1000000"))):
            for value in values:
                monkeypatch.setitem(ctx.options, name, value)
                assert call() == GAT_ERR_ARG, (name, value)
            monkeypatch.delitem(ctx.options, name)
        assert call() == 0
        with pytest.raises(ValueError):
            ctx.efdr_counts(ptr, R, S, dbl, means, [1, 11, 10])
        assert ctx.efdr_times() == (0.0, 0.0)                                        # not asked for: not measured
    finally:
        ctx.free(ptr)


def test_adjust_and_summary_on_the_device_equal_the_model(ctx):
    S = 1000
    m, _, means, obs, k_obs, v, _ = _family(40, S, 0)
    rows = [gat_amd.AnnotatorResult("t", "a%d" % i, "na", o, row) for i, (row, o) in enumerate(zip(m, obs))]
    assert [r.expected for r in rows] == means
    want_q = E.adjusted(k_obs, v, S)
    cutoffs = [0.05, 0.0005, 0.2, 1.0]
    want_rows = E.summary(m, means, obs, cutoffs)
    assert efdr.adjust(rows, ctx=ctx) == want_q
    assert efdr.summary(rows, cutoffs, ctx=ctx) == want_rows
    assert efdr.compute(rows, cutoffs, ctx=ctx) == (want_q, want_rows)
    many = [i / 20.0 for i in range(1, 12)]                                          # 11 cutoffs: two calls of 8 levels at the most
    assert efdr.summary(rows, many, ctx=ctx) == E.summary(m, means, obs, many)
    assert want_rows[3][4:] == ("na", "na", "na") and len(set(want_q)) > 3


def _load(script):
    spec = importlib.util.spec_from_file_location(script.replace("-", "_") + "_efdr", os.path.join(ROOT, "scripts", script + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


INPUTS = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
          "--workspace=%s" % os.path.join(CLI, "workspace.bed")]


def _table(path):
    return [line for line in open(path) if not line.startswith("#")]


def test_cli_efdr_end_to_end(tmp_path):
    """gat-run.py --qvalue-method=efdr --output-stats=fdr_summary on the golden command-line inputs: the first ten columns are the
    golden table's, the qvalue column and the side file are the model applied to the run's own counts file, and the same
    q-values come back through --input-counts-file"""
    mod = _load("gat-run")
    want = _table(os.path.join(CLI, "expected_default.tsv"))
    pattern = str(tmp_path / "counts_%s.tsv")
    out = str(tmp_path / "efdr.tsv")
    assert mod.main(["gat-run.py"] + INPUTS + ["--num-samples=100", "--random-seed=5", "--stdout=%s" % out, "--log=%s" % (tmp_path / "log"),
                                               "--qvalue-method=efdr", "--output-stats=fdr_summary", "--fdr-summary-pvalue=0.05",
                                               "--fdr-summary-pvalue=0.2", "--output-counts-pattern=%s" % pattern,
                                               "--output-filename-pattern=%s" % (tmp_path / "side_%s.tsv")]) == 0
    got = _table(out)
    assert len(got) == len(want) > 2
    assert [line.split("\t")[:10] for line in got] == [line.split("\t")[:10] for line in want]
    assert [line.split("\t")[11:] for line in got] == [line.split("\t")[11:] for line in want]
    rows = gat_amd.fromCounts(pattern % "nucleotide-overlap")
    m = np.stack([r.samples for r in rows])
    means = [float(np.mean(row)) for row in m]
    observed = [r.observed for r in rows]
    _, _, q = E.efdr(m, means, observed)
    model = dict(((r.track, r.annotation), "%6.4e" % x) for r, x in zip(rows, q))
    assert len(model) == len(got) - 1
    for line in got[1:]:
        f = line.split("\t")
        assert f[10] == model[(f[0], f[1])], line
    assert open(str(tmp_path / "side_fdr_summary.tsv")).read() == E.format_summary(E.summary(m, means, observed, [0.05, 0.2]))
    # ... and from the counts file (counter "na", 11 columns)
    again = str(tmp_path / "again.tsv")
    assert mod.main(["gat-run.py", "--input-counts-file=%s" % (pattern % "nucleotide-overlap"), "--qvalue-method=efdr",
                     "--stdout=%s" % again, "--log=%s" % (tmp_path / "log2")]) == 0
    back = dict(((f[0], f[1]), f[10].strip()) for f in (line.split("\t") for line in _table(again)[1:]))
    assert back == model


def test_cli_distance_efdr(tmp_path, monkeypatch):
    """gat-distance.py --qvalue-method=efdr on its golden inputs: the q-values printed are the model's for the rows the script
    handed to the table, whose other columns are those of a --qvalue-method=BH run"""
    mod = _load("gat-distance")
    seen = []
    output = mod.IO.outputResults

    def spy(results, *a, **k):
        seen.append(list(results))
        return output(results, *a, **k)
    monkeypatch.setattr(mod.IO, "outputResults", spy)
    argv = INPUTS + ["--num-samples=50", "--random-seed=11", "--max-distance=300", "--verbose=0"]
    for method in ("efdr", "BH"):
        assert mod.main(["gat-distance.py", "--stdout=%s" % (tmp_path / (method + ".tsv")), "--qvalue-method=%s" % method] + argv) == 0
    got, bh = _table(str(tmp_path / "efdr.tsv")), _table(str(tmp_path / "BH.tsv"))
    assert len(got) == len(bh) > 2
    assert [line.split("\t")[:10] for line in got] == [line.split("\t")[:10] for line in bh]
    rows = seen[0]
    m = np.stack([r.samples for r in rows])
    _, _, q = E.efdr(m, [float(np.mean(row)) for row in m], [r.observed for r in rows])
    model = dict(((r.track, r.annotation), "%6.4e" % x) for r, x in zip(rows, q))
    for line in got[1:]:
        f = line.split("\t")
        assert f[10].strip() == model[(f[0], f[1])], line
