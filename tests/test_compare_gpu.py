"""GPU: k_compare_rows + k_null_stats (gat_compare_stats) against the numpy model (gat_amd.compare.numpy_result, the
reference's own operations), with the device path forced.

What can be equal is equal: the counts of samples below / equal to the observed value -- hence the p-value -- are exact
(the inputs hold no sample whose fc1 / fc2 is within 1e-9 of 1 without being 1: asserted on the model side, for every
pair, none skipped).  The device's log and numpy's each are good to about an ulp and are not the same function, so a
transformed element may differ by e_i = 4 ulp(max(|log r_i|, |delta|)): one ulp for each logarithm, half an ulp for
each addition of delta, a margin of two.  The mean and the standard deviation may then differ by the mean of the e_i
(DESIGN.md section 5 "k_compare_rows"); an order statistic of a row moves by no more than the largest change of an
element, so the two interval values may differ by max e_i."""
import os

import numpy as np
import pytest

import compare_tables as T
import gat_amd
from gat_amd import _lib
from gat_amd import compare as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _results(matrix, observed, prefix):
    return [gat_amd.AnnotatorResult("m", "%s%d" % (prefix, i), "na", float(o), row) for i, (o, row) in enumerate(zip(observed, matrix))]


def _matrix(rs, n_rows, S):
    """counts as a run writes them: integers; row 0 has few distinct values (ties), row 1 is constant"""
    m = rs.randint(20, 6000, (n_rows, S)).astype(np.float64)
    m[0] = rs.choice([300.0, 301.0, 305.0], S)
    m[1] = 777.0
    return m


def _upload(ctx, m):
    ptr = ctx.alloc(m.nbytes)
    ctx.h2d(ptr, m)
    return ptr


def _check(ctx, A, B, pa, pb, ia, ib, pseudo_count, report=None):
    """gat_compare_stats of the pairs (A[ia], B[ib]) against the model, pair by pair"""
    S = A[0].nsamples
    pairs = [C.Pair(0, 1, A[i], B[j], "m", "x") for i, j in zip(ia, ib)]
    st = ctx.compare_stats(pa, len(A), pb, len(B), S, ia, ib, [p.data1.observed for p in pairs], [p.data2.observed for p in pairs],
                           [p.data2.fold - p.data1.fold for p in pairs], pseudo_count)
    worst = 0.0
    for p, got in zip(pairs, st):
        want = C.numpy_result(p, pseudo_count)
        delta = p.data2.fold - p.data1.fold
        r = (p.data1.observed / (p.data1.samples + pseudo_count) + 0.0001) / (p.data2.observed / (p.data2.samples + pseudo_count) + 0.0001)
        assert np.all((np.abs(np.log(r)) > 1e-9) | (r == 1))            # (the premise of the exact counts; holds for every pair)
        s = want.samples
        assert got[6] == 0 and got[7] == 0
        assert (got[4], got[5]) == (np.count_nonzero(s < want.observed), np.count_nonzero(s == want.observed))
        e = 4 * np.spacing(np.maximum(np.abs(np.log(r)), abs(delta)))
        assert abs(got[0] - want.expected) <= e.mean()
        assert abs(got[1] - want.stddev) <= e.mean()
        assert abs(got[2] - want.lower95) <= e.max() and abs(got[3] - want.upper95) <= e.max()
        worst = max(worst, abs(got[0] - want.expected) / e.mean(), abs(got[1] - want.stddev) / e.mean(),
                    abs(got[2] - want.lower95) / e.max(), abs(got[3] - want.upper95) / e.max())
        res = gat_amd.AnnotatorResult("m", "x", "na", want.observed, s, reference=None, pseudo_count=0, _stats=tuple(got[:6]))
        assert res.pvalue == want.pvalue
    print("S=%d pairs=%d: largest deviation / bound = %.3f" % (S, len(pairs), worst))
    return worst


@pytest.mark.parametrize("n_pairs", [1, 3, 130])
@pytest.mark.parametrize("S", [1, 2, 19, 20, 64, 65, 257, 8193])
def test_compare_stats_equal_the_model(ctx, S, n_pairs, monkeypatch):
    rs = np.random.RandomState(1000 * S + n_pairs)
    ma, mb = _matrix(rs, 9, S), _matrix(rs, 7, S)
    A, B = _results(ma, rs.randint(100, 5000, 9), "a"), _results(mb, rs.randint(100, 5000, 7), "b")
    pa, pb = _upload(ctx, ma), _upload(ctx, mb)
    # 48 rows of scratch (rows have an even stride): 130 pairs are batches of 48, 48 and 34
    stride = S + (S & 1)
    monkeypatch.setitem(ctx.options, "GAT_COMPARE_SCRATCH_MB", repr(48.5 * stride * 8 / 2.0 ** 20))
    try:
        ia, ib = rs.randint(0, 9, n_pairs), rs.randint(0, 7, n_pairs)
        ia[0], ib[0] = 0, 1                                             # the row of ties against the constant row
        if n_pairs > 1:
            ia[1], ib[1] = 1, 1                                         # constant against constant: a constant transformed row
            ia[-1], ib[-1] = 8, 6                                       # the last rows of both, in the ragged batch
        _check(ctx, A, B, pa, pb, ia, ib, 1.0)
        # one matrix on both sides, ia == ib among the pairs: fc1 / fc2 is exactly 1, the row all zeros
        ia2 = rs.randint(0, 9, n_pairs)
        ib2 = np.where(np.arange(n_pairs) % 2 == 0, ia2, rs.randint(0, 9, n_pairs))
        _check(ctx, A, A, pa, pa, ia2, ib2, 0.5)
        k = int(np.flatnonzero(ia2 == ib2)[0])
        st = ctx.compare_stats(pa, 9, pa, 9, S, ia2[k:k + 1], ib2[k:k + 1], [A[ia2[k]].observed], [A[ia2[k]].observed], [0.0], 0.5)
        assert st[0, :6].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, float(S)]
    finally:
        ctx.free(pa)
        ctx.free(pb)


def _large_case(S):
    """the matrices, results and three pairs of test_compare_stats_at_large_sample_counts (seed 1000 * S + 3: no sample of the
    three pairs has a fold ratio within 1e-9 of 1 without being 1, which _check asserts on the host for each pair)"""
    rs = np.random.RandomState(1000 * S + 3)
    ma, mb = _matrix(rs, 9, S), _matrix(rs, 7, S)
    A, B = _results(ma, rs.randint(100, 5000, 9), "a"), _results(mb, rs.randint(100, 5000, 7), "b")
    return ma, mb, A, B, [0, 1, 8], [1, 1, 6]      # ties against constant, constant against constant, the last rows of both


@pytest.mark.parametrize("S", [24577, 40961])
def test_compare_stats_at_large_sample_counts(ctx, S):
    """k_compare_rows feeding k_null_stats where np_sum has the partial chunk on wave 3 (three full chunks of 8 192 and one
    element) and where its waves take a second full chunk (five and one element); the bounds are _check's, unchanged"""
    ma, mb, A, B, ia, ib = _large_case(S)
    pa, pb = _upload(ctx, ma), _upload(ctx, mb)
    try:
        _check(ctx, A, B, pa, pb, ia, ib, 1.0)
    finally:
        ctx.free(pa)
        ctx.free(pb)


def test_bad_arguments(ctx):
    m = np.ones((3, 8))
    p = _upload(ctx, m)
    try:
        for ia, ib in (([3], [0]), ([0], [-1])):                        # a row outside its matrix
            with pytest.raises(ValueError):
                ctx.compare_stats(p, 3, p, 3, 8, ia, ib, [1.0], [1.0], [0.0], 1.0)
        assert ctx.compare_stats(p, 3, p, 3, 8, [], [], [], [], [], 1.0).shape == (0, 8)
    finally:
        ctx.free(p)


def test_zero_counts_without_pseudo_count_fall_back_to_numpy(ctx, monkeypatch):
    """pseudo_count = 0 against a zero count: inf, or nan from inf / inf, as numpy gives them; the pair's non-finite samples
    are counted (slot 6) and compare() recomputes exactly those pairs on the host"""
    monkeypatch.setenv("GAT_DEVICE_STATS", "1")
    rs = np.random.RandomState(5)
    m = rs.randint(20, 900, (5, 65)).astype(np.float64)
    m[1, [0, 7, 64]] = 0.0
    m[3, [7, 30]] = 0.0
    rows = _results(m, rs.randint(100, 900, 5), "a")
    p = _upload(ctx, m)
    try:
        pairs = C.pairs_of([rows])
        st = ctx.compare_stats(p, 5, p, 5, 65, [int(q.track[1:]) for q in pairs], [int(q.annotation[1:]) for q in pairs],
                               [q.data1.observed for q in pairs], [q.data2.observed for q in pairs],
                               [q.data2.fold - q.data1.fold for q in pairs], 0.0)
    finally:
        ctx.free(p)
    want_bad = [len(set(np.flatnonzero(q.data1.samples == 0)) | set(np.flatnonzero(q.data2.samples == 0))) for q in pairs]
    assert st[:, 6].tolist() == want_bad and sorted(set(want_bad)) == [0, 2, 3, 4]
    got, want = C.compare([rows], pseudo_count=0.0, ctx=ctx), C.compare_numpy([rows], pseudo_count=0.0)
    assert len(got) == len(want) == 10
    for g, w, bad in zip(got, want, want_bad):
        assert (g._raw is None) == (bad > 0)                            # built from the device's numbers unless recomputed
        if bad:
            assert str(g) == str(w)
        else:
            assert g.pvalue == w.pvalue and abs(g.expected - w.expected) < 1e-12


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_script_on_the_device_prints_the_reference_table(name, tmp_path, monkeypatch):
    monkeypatch.setenv("GAT_DEVICE_STATS", "1")
    seen = []
    real = _lib.Context.compare_stats
    monkeypatch.setattr(_lib.Context, "compare_stats", lambda self, *a: seen.append(len(a[5])) or real(self, *a))
    got, want = T.run_case(T.script(), name, str(tmp_path / "out.tsv"))
    assert sum(seen) == len(want) - 1                                   # every pair went through gat_compare_stats
    T.assert_tables_match(got, want)


def test_thousand_random_pairs_of_500_samples(ctx, monkeypatch):
    rs = np.random.RandomState(77)
    ma, mb = _matrix(rs, 40, 500), _matrix(rs, 40, 500)
    A, B = _results(ma, rs.randint(100, 5000, 40), "a"), _results(mb, rs.randint(100, 5000, 40), "b")
    pa, pb = _upload(ctx, ma), _upload(ctx, mb)
    try:
        _check(ctx, A, B, pa, pb, rs.randint(0, 40, 1000), rs.randint(0, 40, 1000), 1.0)
    finally:
        ctx.free(pa)
        ctx.free(pb)


def test_compare_through_the_device_and_lazy_samples(ctx, monkeypatch):
    """compare() with the device forced: the same list as the numpy path, rows only on demand"""
    monkeypatch.setenv("GAT_DEVICE_STATS", "1")
    rs = np.random.RandomState(9)
    rows = _results(_matrix(rs, 12, 257), rs.randint(100, 5000, 12), "a")
    got, want = C.compare([rows], ctx=ctx), C.compare_numpy([rows])
    assert len(got) == 66
    for g, w in zip(got, want):
        assert (g.track, g.annotation, g.observed, g.pvalue, g.nsamples) == (w.track, w.annotation, w.observed, w.pvalue, w.nsamples)
        assert g._samples_cache is None and abs(g.expected - w.expected) < 1e-13 and abs(g.stddev - w.stddev) < 1e-13
    assert np.array_equal(got[5].samples, want[5].samples)
    # two files of different tracks / annotations sets, each uploaded once
    f0 = _results(_matrix(rs, 6, 64), rs.randint(100, 5000, 6), "a")
    f1 = list(reversed(_results(_matrix(rs, 6, 64), rs.randint(100, 5000, 6), "a")))[:4]
    got, want = C.compare([f0, f1], ctx=ctx), C.compare_numpy([f0, f1])
    assert [(g.annotation, g.pvalue) for g in got] == [(w.annotation, w.pvalue) for w in want] and len(got) == 4
