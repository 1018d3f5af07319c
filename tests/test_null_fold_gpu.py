"""GPU: gat_null_fold (k_null_fold) against the integer models of tests/null_fold_model.py -- matrices uploaded, not sampled,
so that the numbers are chosen; the eight words of every row have to equal the model's -- and the deep run end to end:
scripts/gat-run.py --null-round-size on the golden command-line inputs, gat_amd.run(null_round_size=...) against the rows of
the plain run."""
import ctypes
import importlib.util
import os
from decimal import Decimal

import numpy as np
import pytest

import gat_amd
import null_fold_model as M
from gat_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
SHAPES = ("default", "1", "2", "7", "1024")          # GAT_NULL_FOLD_PARTS: every launch shape there is
PAD = (1 << 62) + 12345                              # what lies in the slots between the rows: a read of it shows in every word


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


class _Device(object):
    """a matrix on the device, rows `stride` slots apart and `lead` slots into the allocation (an odd lead or stride: rows
    that do not start on a 16-byte boundary), PAD everywhere else; and the words of its rows"""

    def __init__(self, ctx, m, stride=None, lead=0):
        self.ctx, (self.n_rows, self.n) = ctx, m.shape
        self.stride = self.n if stride is None else stride
        slots = np.full(lead + self.n_rows * self.stride + 2, PAD, dtype=np.uint64)
        body = slots[lead:lead + self.n_rows * self.stride].reshape(self.n_rows, self.stride)
        body[:, :self.n] = m
        self.base = ctx.alloc(slots.nbytes)
        self.words_ptr = ctx.alloc(max(1, self.n_rows) * 64)
        ctx.h2d(self.base, slots)
        self.ptr = self.base + 8 * lead

    def reset(self):
        self.ctx.null_fold_reset(self.words_ptr, self.n_rows)

    def fold(self, vals, first=0, n=None):
        """samples [first, first + n) of every row"""
        n = self.n - first if n is None else n
        self.ctx.null_fold(self.ptr + 8 * first, self.n_rows, n, self.stride, vals, self.words_ptr)

    def words(self):
        return self.ctx.null_fold_words(self.words_ptr, self.n_rows)

    def close(self):
        self.ctx.free(self.words_ptr)
        self.ctx.free(self.base)


def _shape(ctx, monkeypatch, shape):
    if shape != "default":
        monkeypatch.setitem(ctx.options, "GAT_NULL_FOLD_PARTS", shape)
    elif "GAT_NULL_FOLD_PARTS" in ctx.options:
        monkeypatch.delitem(ctx.options, "GAT_NULL_FOLD_PARTS")


def _vals(m, rs):
    """per row, in turn: below the minimum, above the maximum, on a value of the row, on x.5, 0, 1e30 (clamped)"""
    out = []
    for r, row in enumerate(m):
        kind = r % 6
        out.append([float(row.min()) - 1.0, float(row.max()) + 1.0, float(row[int(rs.randint(len(row)))]),
                    float(row[0] >> np.uint64(1)) + 0.5, 0.0, 1e30][kind])
    return out


_CASES = {}


def _case(n_rows, n):
    """a shape's matrix, values and model words, made once and shared by the strides and launch shapes; values below 2^40
    (a double holds them: `vals` can sit on one exactly) with ties: every fourth row has eight distinct values"""
    if (n_rows, n) not in _CASES:
        rs = np.random.RandomState(1000003 * n_rows + n)
        m = rs.randint(0, 1 << 40, (n_rows, n)).astype(np.uint64)
        m[::4] &= np.uint64(7)
        vals = _vals(m, rs)
        want = M.words_numpy(m, vals)
        m.setflags(write=False)
        _CASES[(n_rows, n)] = (m, vals, want)
    return _CASES[(n_rows, n)]


@pytest.mark.parametrize("n_rows", [1, 2, 3, 257])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 100003])
def test_words_equal_the_model(ctx, n, n_rows, monkeypatch):
    """every wave and workgroup edge of a row, one row and several and more than one launch fills, rows that start on and off a
    16-byte boundary (stride n, n + 1, n + 2 from an even and an odd first slot), under every launch shape"""
    m, vals, want = _case(n_rows, n)
    for stride, lead in ((n, 0), (n + 1, 0), (n + 2, 1), (n, 1)):
        d = _Device(ctx, m, stride, lead)
        try:
            for shape in SHAPES:
                _shape(ctx, monkeypatch, shape)
                d.reset()
                d.fold(vals)
                got = d.words()
                assert got == want, "n=%d rows=%d stride=%d lead=%d parts=%s: row %d" % (
                    n, n_rows, stride, lead, shape, next(r for r in range(n_rows) if got[r] != want[r]))
        finally:
            d.close()


def test_the_numpy_model_agrees_with_the_python_model_on_a_case():
    m, vals, want = _case(3, 257)
    assert want == M.words(m.tolist(), vals)


VALUE_CASES = {
    "zeros": lambda rs, n: np.zeros(n, dtype=np.uint64),
    "around 2^32": lambda rs, n: np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + 1], dtype=np.uint64)[rs.randint(0, 3, n)],
    "near 2^62": lambda rs, n: ((1 << 62) - rs.randint(1, 1 << 20, n)).astype(np.uint64),
    "2^63 - 1": lambda rs, n: np.full(n, (1 << 63) - 1, dtype=np.uint64),
}


@pytest.mark.parametrize("kind", sorted(VALUE_CASES))
@pytest.mark.parametrize("n", [9, 1000, 5003])
def test_values_where_the_product_needs_128_bits(ctx, kind, n, monkeypatch):
    """0 only; 2^32 - 1, 2^32, 2^32 + 1, where the product's high half comes alive; values near 2^62, whose squares wrap the
    low word several times in one call (nine samples: the high word still holds the sum; 1000 and 5003: it wraps too, the sum
    is modulo 2^128); and the same matrix folded a second time into the same words: the carry crosses the calls"""
    rs = np.random.RandomState(n)
    m = np.stack([VALUE_CASES[kind](rs, n) for _ in range(3)])
    vals = [float(m[0, 0]), float(m[1].min()) - 0.5, 1e30]
    once = M.words(m.tolist(), vals)
    if kind == "near 2^62":
        for r in range(3):
            exact = sum(int(v) ** 2 for v in m[r].tolist())
            assert sum((int(v) ** 2) & M.M64 for v in m[r].tolist()) >> 64 >= 2      # the low word wraps more than once
            assert once[r][2:4] == (exact & M.M64, (exact >> 64) & M.M64)
    twice = [M.add(w, w) for w in once]
    d = _Device(ctx, m, n + 1, 1)
    try:
        for shape in SHAPES:
            _shape(ctx, monkeypatch, shape)
            d.reset()
            d.fold(vals)
            assert d.words() == once, (kind, n, shape)
            d.fold(vals)
            assert d.words() == twice, (kind, n, shape)
    finally:
        d.close()


@pytest.mark.parametrize("n", [2, 65, 4097])
def test_every_kind_of_value_asked_for(ctx, n):
    """val below the minimum, above the maximum, on a tie that fills the row, on x.5, 0, 1e30 (clamped), negative, -0.0, and
    an integer beyond 2^63"""
    rs = np.random.RandomState(n)
    vals = [4.0, 100.0, 7.0, 6.5, 0.0, 1e30, -2.0, -0.0, 2.0 ** 63, 5.0, 0.5]
    m = rs.randint(5, 100, (len(vals), n)).astype(np.uint64)
    m[2] = 7                                                              # the tie that fills the row
    m[4, ::2] = 0
    m[7, 1::2] = 0
    m[9, : n // 2] = 5
    want = M.words(m.tolist(), vals)
    assert want[2][5] == n and want[0][4] == 0 and want[1][4] == n and want[5][4] == n and want[8][4] == n and want[6][4:6] == (0, 0)
    assert want[4][5] == (n + 1) // 2 and want[7][5] == n // 2
    d = _Device(ctx, m)
    try:
        d.reset()
        d.fold(vals)
        assert d.words() == want
    finally:
        d.close()


@pytest.mark.parametrize("n,half", [(2, 1), (65, 1), (257, 64), (4097, 2049), (100003, 50001)])
def test_two_folds_of_halves_are_the_fold_of_the_whole(ctx, n, half, monkeypatch):
    """rounds of a run: [0, half) and [half, n) of rows n slots apart, in both orders, against one fold"""
    m, vals, want = _case(3, n)
    d = _Device(ctx, m)
    try:
        for shape in ("default", "7"):
            _shape(ctx, monkeypatch, shape)
            for order in ((0, half), (half, 0)):
                d.reset()
                for first in order:
                    d.fold(vals, first, half if first == 0 else n - half)
                assert d.words() == want, (n, half, shape, order)
    finally:
        d.close()


def test_more_rows_than_one_launch(ctx):
    """2^20 + 5 rows of two samples, three slots apart: gat_null_fold's second launch and its four offset pointers (the matrix,
    the two integer parameters, the words); every word of every row, the model vectorised (values below 2^20: nothing wraps)"""
    n_rows, n = (1 << 20) + 5, 2
    rs = np.random.RandomState(77)
    m = rs.randint(0, 1 << 20, (n_rows, n)).astype(np.uint64)
    vals = rs.randint(0, 1 << 20, n_rows).astype(np.float64)
    vals[::3] = m[::3, 1]                                                  # a third of the rows asked for a value they hold
    v = vals.astype(np.uint64)[:, None]
    want = np.stack([np.full(n_rows, n, dtype=np.uint64), m.sum(axis=1), (m * m).sum(axis=1), np.zeros(n_rows, dtype=np.uint64),
                     (m < v).sum(axis=1).astype(np.uint64), (m == v).sum(axis=1).astype(np.uint64), m.min(axis=1), m.max(axis=1)], axis=1)
    for r in (0, 1, (1 << 20) - 1, 1 << 20, n_rows - 1):                   # the vectorised model against the Python one
        assert tuple(int(x) for x in want[r]) == M.row_words(m[r].tolist(), float(vals[r]))
    d = _Device(ctx, m, 3, 0)
    try:
        d.reset()
        d.fold(vals)
        got = np.zeros((n_rows, 8), dtype=np.uint64)
        ctx.d2h(got, d.words_ptr)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "rows %s ...: %s, model %s" % (bad[:5], got[bad[0]], want[bad[0]])
    finally:
        d.close()


def test_reset_alone(ctx):
    d = _Device(ctx, np.zeros((5, 3), dtype=np.uint64))
    try:
        ctx.h2d(d.words_ptr, np.full(5 * 8, 77, dtype=np.uint64))
        d.reset()
        assert d.words() == [M.EMPTY] * 5 and M.EMPTY[0] == 0 and M.EMPTY[6] == (1 << 64) - 1
    finally:
        d.close()


def test_errors_and_no_rows(ctx, monkeypatch):
    L = _lib.lib()
    d = _Device(ctx, np.arange(12, dtype=np.uint64).reshape(3, 4))
    vals = np.array([1.0, 2.0, 3.0])

    def fold(counts=d.ptr, n_rows=3, n=4, stride=4, v=vals, words=d.words_ptr, h=ctx._h):
        return L.gat_null_fold(h, ctypes.c_void_p(counts), n_rows, n, stride, v.ctypes.data_as(ctypes.c_void_p) if v is not None else None,
                               ctypes.c_void_p(words))
    try:
        d.reset()
        before = d.words()
        ARG = -6                                                          # GAT_ERR_ARG
        assert fold(h=None) == ARG and fold(counts=None) == ARG and fold(v=None) == ARG and fold(words=None) == ARG
        assert fold(n=0) == ARG and fold(n=-1) == ARG and fold(stride=3) == ARG and fold(n_rows=-1) == ARG
        for bad in (np.nan, np.inf, -np.inf):
            assert fold(v=np.array([1.0, bad, 3.0])) == ARG
            assert b"row 1 is not finite" in L.gat_last_error(ctx._h)
        with pytest.raises(ValueError, match="row 1 is not finite"):
            ctx.null_fold(d.ptr, 3, 4, 4, [1.0, float("nan"), 3.0], d.words_ptr)
        assert L.gat_null_fold_reset(None, ctypes.c_void_p(d.words_ptr), 3) == ARG
        assert L.gat_null_fold_reset(ctx._h, None, 3) == ARG and L.gat_null_fold_reset(ctx._h, ctypes.c_void_p(d.words_ptr), -1) == ARG
        monkeypatch.setitem(ctx.options, "GAT_NULL_FOLD_PARTS", "1025")
        assert fold() == ARG and b"GAT_NULL_FOLD_PARTS" in L.gat_last_error(ctx._h)
        monkeypatch.setitem(ctx.options, "GAT_NULL_FOLD_PARTS", "-1")
        assert fold() == ARG
        monkeypatch.delitem(ctx.options, "GAT_NULL_FOLD_PARTS")
        assert d.words() == before                                        # nothing was touched
        assert fold(n_rows=0) == 0 and L.gat_null_fold_reset(ctx._h, ctypes.c_void_p(d.words_ptr), 0) == 0
        assert d.words() == before
        assert fold() == 0
        assert d.words() == M.words(np.arange(12).reshape(3, 4).tolist(), vals.tolist())
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------
# end to end

def _run_cli(tmp_path, tag, extra, num_samples=100):
    spec = importlib.util.spec_from_file_location("gat_run_deep", os.path.join(ROOT, "scripts", "gat-run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / ("%s.tsv" % tag))
    argv = ["gat-run.py", "--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
            "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=%d" % num_samples, "--random-seed=5",
            "--stdout=%s" % out, "--log=%s" % str(tmp_path / ("%s.log" % tag))] + extra
    assert mod.main(argv) == 0
    return [line for line in open(out) if not line.startswith("#")]


CI_LOW, CI_HIGH, STDDEV = 4, 5, 6


def _fields(lines):
    return [line.rstrip("\n").split("\t") for line in lines]


def _without(fields, columns):
    return [[f for i, f in enumerate(row) if i not in columns] for row in fields]


@pytest.fixture(scope="module")
def deep32(tmp_path_factory):
    """gat-run.py --null-round-size=32 on the golden inputs, and the rounds it enqueued"""
    rounds = []
    enqueue = _lib.Problem.enqueue

    def recording(self, counters, seed, sample_begin, sample_end, counts_dev_ptr):
        rounds.append((sample_begin, sample_end))
        return enqueue(self, counters, seed, sample_begin, sample_end, counts_dev_ptr)
    _lib.Problem.enqueue = recording
    try:
        tmp = tmp_path_factory.mktemp("deep32")
        table = _fields(_run_cli(tmp, "deep32", ["--null-round-size=32"]))
    finally:
        _lib.Problem.enqueue = enqueue
    return table, rounds, open(str(tmp / "deep32.log")).read()


def test_cli_rounds_and_table(deep32, tmp_path):
    table, rounds, log = deep32
    assert rounds == [(0, 32), (32, 64), (64, 96), (96, 100)]
    assert "CI95low and CI95high are the interval of the first round's 32 samples" in log
    want = _fields(line for line in open(os.path.join(CLI, "expected_default.tsv")) if not line.startswith("#"))
    assert len(table) == len(want) > 2 and table[0] == want[0]
    assert table[0][CI_LOW:STDDEV + 1] == ["CI95low", "CI95high", "stddev"]
    # track, annotation, observed, expected, fold, l2fold, pvalue, qvalue and every column behind them: byte for byte
    assert _without(table, (CI_LOW, CI_HIGH, STDDEV)) == _without(want, (CI_LOW, CI_HIGH, STDDEV))
    for got, w in zip(table[1:], want[1:]):
        print("stddev %s (golden %s)" % (got[STDDEV], w[STDDEV]))
        assert got[STDDEV] == w[STDDEV] or abs(Decimal(got[STDDEV].strip()) - Decimal(w[STDDEV].strip())) == Decimal("0.0001"), (got, w)
    # the interval is the first round's: that of a plain run of the same command with 32 samples
    first = _fields(_run_cli(tmp_path, "plain32", [], num_samples=32))
    assert [row[:2] + row[CI_LOW:CI_HIGH + 1] for row in table] == [row[:2] + row[CI_LOW:CI_HIGH + 1] for row in first]


@pytest.mark.parametrize("size", [1, 100, 1000])
def test_cli_round_size_changes_nothing_but_the_interval(deep32, size, tmp_path):
    got = _fields(_run_cli(tmp_path, "deep%d" % size, ["--null-round-size=%d" % size]))
    assert _without(got, (CI_LOW, CI_HIGH)) == _without(deep32[0], (CI_LOW, CI_HIGH))
    if size >= 100:                                                           # one round: the plain run's interval
        want = _fields(line for line in open(os.path.join(CLI, "expected_default.tsv")) if not line.startswith("#"))
        assert [row[CI_LOW:CI_HIGH + 1] for row in got] == [row[CI_LOW:CI_HIGH + 1] for row in want]


def test_run_rows_hold_the_words_of_the_plain_runs_samples():
    """every integer counter (nucleotide-density, the sixth, has float rows and is refused): gat_amd.run(null_round_size=7) --
    fifteen rounds, the last of two samples -- against the model applied to the samples the plain run kept"""
    counters = [n for n in gat_amd.COUNTERS if n != "nucleotide-density"]
    assert len(counters) == 5

    def rows(null_round_size):
        argv = ["--segments=%s" % os.path.join(CLI, "segments.bed"), "--annotations=%s" % os.path.join(CLI, "annotations.bed"),
                "--workspace=%s" % os.path.join(CLI, "workspace.bed"), "--num-samples=100", "--random-seed=5",
                "--null-round-size=%d" % null_round_size] + ["--counter=%s" % c for c in counters]
        options, args = gat_amd.buildParser().parse_args(argv)
        return gat_amd.fromSegments(options, args)
    plain, deep = rows(0), rows(7)
    assert len(plain) == len(deep) >= 2 * len(counters)
    assert sorted(set(r.counter for r in deep)) == sorted(counters)
    for p, d in zip(plain, deep):
        assert (p.track, p.annotation, p.counter, p.observed) == (d.track, d.annotation, d.counter, d.observed)
        assert p.null_words is None
        w = M.row_words([int(v) for v in p.samples.tolist()], p.observed)
        assert d.null_words == w, (d.counter, d.annotation)
        model = M.row(w, d.observed)
        assert (d.nsamples, d.expected, d.stddev, d.pvalue) == (100, model["expected"], model["stddev"], model["pvalue"])
        assert (d.expected, d.pvalue, d.fold) == (p.expected, p.pvalue, p.fold)
        assert str(d).split("\t")[7:] == str(p).split("\t")[7:]
        with pytest.raises(ValueError, match="never kept"):
            d.samples
