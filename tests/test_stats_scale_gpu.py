"""GPU: the statistics kernels at the sample and row counts a production run has -- k_null_stats (gat_null_stats) and
k_minp_rank / k_minp_step (gat_minp_counts), through gat_amd._lib only.

What the smaller shapes of tests/test_hip_parity.py and tests/test_minp_gpu.py do not reach:
  * np_sum's wave-strided loop over full chunks of 8 192 (a second trip from S = 40 960), the partial chunk on wave 3
    (three full chunks in front of it), rows of negative and mixed-sign values, interval positions other than the wrapper's;
  * gat_null_stats' second launch (more than 2^20 rows);
  * k_minp_rank's grid-stride loop (more than 512 rows: a workgroup's second and third row, with its buffers reused; the
    cases of 300 samples are the ones whose counts depend on those rows, see _minp_rows_case), the
    switch between the LDS and the global-memory sort at the default and at the largest GAT_MINP_LDS_SAMPLES, rows of
    65 537 and 100 003 samples (391 keys per thread, the last threads without any).

Every comparison is equality: the sums bit for bit against numpy through AnnotatorResult, order statistics and counts
against numpy's sort, minP counts against tests/minp_model.py.  The double rows are order sensitive -- their numpy mean
differs from the left-to-right one -- which each test asserts before it looks at the device: a kernel adding in another
order than numpy cannot pass on them.  (Integer rows below 2^53 / S sum exactly in any order and carry none of that.)
Signed zeros and non-finite values are kept out of the k_null_stats rows: numpy's sort leaves the order of -0.0 and 0.0 open."""
import ctypes
import re

import numpy as np
import pytest

import gat_amd
import minp_model as M
from gat_amd import _lib

gpu = pytest.mark.gpu

GAT_ERR_ARG = -6
STATS_S = [24577, 32767, 32768, 40960, 40961, 65665, 100000, 250000]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# k_null_stats: sums


def _order_sensitive(row):
    return float(np.mean(row)) != float(np.cumsum(row)[-1] / len(row))


def _stats_rows(S):
    """(rows as float64, is_double) of test_device_null_stats_equal_numpy's five kinds, a double row of mixed sign, one that
    is all negative and an int64 row with negative entries.  Seed S + 3: the first offset at which the four double rows are
    order sensitive at every S of STATS_S (at offsets 0, 1 and 2 one of the 32 rows has both means equal: the division rounds
    the difference of the sums away); test_sum_premises_hold, which needs no device, and the device test itself assert it"""
    rs = np.random.RandomState(S + 3)
    rows = [rs.randint(0, 50, S).astype(np.float64),                    # ties everywhere
            rs.randint(0, 10 ** 7, S).astype(np.float64),
            rs.random_sample(S) * 1e5,                                  # IEEE doubles (density)
            np.full(S, 7.0),                                            # constant
            np.abs(rs.standard_cauchy(S) * 1e3),                        # heavy tail, doubles
            rs.normal(0, 1e3, S),                                       # doubles of mixed sign
            -(rs.random_sample(S) * 1e5 + 1.0),                         # doubles, all negative
            rs.randint(-10 ** 6, 10 ** 6, S).astype(np.float64)]       # int64 with negative entries
    is_double = np.array([0, 0, 1, 0, 1, 1, 1, 0], dtype=np.uint8)
    return rows, is_double


def _slots(rows, is_double):
    """the rows as gat_null_stats' layout holds them: 8-byte slots, int64, or the double's bits for the flagged rows"""
    out = np.zeros((len(rows), len(rows[0])), dtype=np.int64)
    for r, row in enumerate(rows):
        if is_double[r]:
            out[r] = np.ascontiguousarray(row, dtype=np.float64).view(np.int64)
        else:
            assert np.array_equal(row, np.round(row))
            out[r] = np.asarray(row).astype(np.int64)
    return out


def _observed(rows):
    """four observed values per row: below the row, on a value of the row, inside it off its values, above it"""
    below = [float(r.min()) - 1.0 for r in rows]
    member = [float(r[len(r) // 3]) for r in rows]
    inside = []
    for r in rows:
        u = np.unique(r)
        inside.append(float(u[len(u) // 2 - 1] + u[len(u) // 2]) / 2 if len(u) > 1 else float(u[0]) + 0.5)
    above = [float(r.max()) + 1.0 for r in rows]
    return [below, member, inside, above]


def _check_premises(S, rows, is_double, observed):
    assert [i for i in range(len(rows)) if is_double[i]] == [2, 4, 5, 6]
    for i in (2, 4, 5, 6):
        assert _order_sensitive(rows[i]), (S, i)                        # a sum in another order is another number
        assert np.all(np.isfinite(rows[i])) and not np.any(rows[i] == 0)
    assert rows[5].min() < 0 < rows[5].max() and rows[6].max() < 0 and rows[7].min() < 0 < rows[7].max()
    below, member, inside, above = observed
    for r, row in enumerate(rows):
        assert below[r] < row.min() and above[r] > row.max() and np.any(row == member[r])
        if row.min() < row.max():
            assert row.min() < inside[r] < row.max() and not np.any(row == inside[r])


@pytest.mark.parametrize("S", STATS_S)
def test_sum_premises_hold(S):
    """no device: the rows of test_null_stats_sums_equal_numpy are what it says they are, at every S"""
    rows, is_double = _stats_rows(S)
    _check_premises(S, rows, is_double, _observed(rows))
    chunks = {24577: (3, 1), 32767: (3, 8191), 32768: (4, 0), 40960: (5, 0), 40961: (5, 1), 65665: (8, 129), 100000: (12, 1696),
              250000: (30, 4240)}
    assert divmod(S, 8192) == chunks[S]                                 # (full chunks, elements of the partial one)


@gpu
@pytest.mark.parametrize("S", STATS_S)
def test_null_stats_sums_equal_numpy(ctx, S):
    """gat_null_stats against AnnotatorResult's numpy, bit for bit, where np_sum takes more than one trip of its chunk loop
    and where the partial chunk lands on wave 3; rows of either sign; observed values below, on, inside and above each row"""
    rows, is_double = _stats_rows(S)
    observed = _observed(rows)
    _check_premises(S, rows, is_double, observed)
    mat = _slots(rows, is_double)
    dev = ctx.alloc(mat.nbytes)
    try:
        ctx.h2d(dev, mat)
        stats = [ctx.null_stats(dev, len(rows), S, is_double, np.array(vals)) for vals in observed]
    finally:
        ctx.free(dev)
    for vals, st in zip(observed, stats):
        for r in range(len(rows)):
            host = gat_amd.AnnotatorResult("t", "a", "c", vals[r], rows[r])
            devr = gat_amd.AnnotatorResult("t", "a", "c", vals[r], rows[r], _stats=tuple(st[r, :6]))
            for f in ("expected", "stddev", "lower95", "upper95", "fold", "pvalue"):
                assert getattr(host, f) == getattr(devr, f), (S, r, vals[r], f, getattr(host, f), getattr(devr, f))
            assert str(host) == str(devr)


# ---------------------------------------------------------------------------------------------------------------------
# k_null_stats: order statistics at chosen positions, through the C ABI


def _null_stats_abi(ctx, dev, n_rows, S, is_double, vals, lo, hi):
    out = np.full((n_rows, 8), -7.0)
    is_double = np.ascontiguousarray(is_double, dtype=np.uint8)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.lib().gat_null_stats(ctx._h, ctypes.c_void_p(dev), n_rows, S, p(is_double), p(vals), lo, hi, p(out))
    assert rc == 0, _lib.lib().gat_last_error(ctx._h)
    return out


@gpu
@pytest.mark.parametrize("S", [1, 2, 257, 40961])
def test_order_statistics_at_chosen_positions(ctx, S):
    """slots 2 .. 5 of gat_null_stats for the first and the last position, the two swapped, one position twice and the two
    around the middle: the sorted row's values exactly, on rows of ties, a constant row and doubles of either sign"""
    rs = np.random.RandomState(77 + S)
    rows = [rs.randint(-3, 4, S).astype(np.float64),                    # heavy ties, either sign
            np.full(S, -7.0),                                           # constant
            rs.normal(0, 1e3, S),                                       # doubles of mixed sign
            -(rs.random_sample(S) * 1e5 + 1.0)]                         # doubles, all negative
    is_double = np.array([0, 0, 1, 1], dtype=np.uint8)
    assert all(np.all(np.isfinite(r)) and not np.any(r == 0) for r in rows[2:])
    if S > 2:
        assert rows[2].min() < 0 < rows[2].max() and len(np.unique(rows[0])) == 7
    srt = [np.sort(r) for r in rows]
    k = S // 3
    positions = [(0, S - 1), (S - 1, 0), (k, k), (S // 2, min(S // 2 + 1, S - 1))]
    observed = _observed(rows)
    mat = _slots(rows, is_double)
    dev = ctx.alloc(mat.nbytes)
    try:
        ctx.h2d(dev, mat)
        for n, (lo, hi) in enumerate(positions):
            vals = observed[(n + 1) % 4]                                # (on a value of the row for the first pair)
            out = _null_stats_abi(ctx, dev, len(rows), S, is_double, vals, lo, hi)
            for r, row in enumerate(rows):
                want = [float(srt[r][lo]), float(srt[r][hi]), float(np.count_nonzero(row < vals[r])), float(np.count_nonzero(row == vals[r]))]
                assert out[r, 2:6].tolist() == want, (S, lo, hi, r, out[r].tolist(), want)
                assert np.signbit(out[r, 2]) == np.signbit(want[0]) and np.signbit(out[r, 3]) == np.signbit(want[1])
                assert out[r, 0] == float(np.mean(row)) and out[r, 6] == 0 and out[r, 7] == 0
    finally:
        ctx.free(dev)


# ---------------------------------------------------------------------------------------------------------------------
# gat_null_stats: more rows than one launch takes


FIRST_LAUNCH = 1 << 20                                                  # rows of one launch of k_null_stats


def _many_rows():
    """(m, is_double, vals, want) of 2^20 + 5 rows of two samples: int64 and double rows alternating in blocks of 11, vals drawn
    per row (below, on either sample, between them, above), and all eight slots of every row from numpy over the whole
    matrix -- two numbers add to the same bits in any order, so the expression is exact.  The six rows around the boundary
    hold values no other row has, and the flags of the five rows behind it differ from those of rows 0 .. 4: a launch that
    reads or writes without its offset meets other numbers."""
    first = FIRST_LAUNCH
    R = first + 5
    rs = np.random.RandomState(20)
    is_double = ((np.arange(R) // 11) % 2).astype(np.uint8)
    assert np.all(is_double[first:] != is_double[:5])
    ints = rs.randint(-1000, 1000, (R, 2)).astype(np.float64)
    dbls = np.round(rs.normal(0, 300, (R, 2)), 2)
    dbls[dbls == 0] = 0.25                                              # (no signed zeros)
    m = np.where(is_double[:, None] != 0, dbls, ints)
    edge = np.arange(first - 1, R)
    for j, r in enumerate(edge):
        m[r] = (2e6 + 17.25 * j, 2e6 + 17.25 * j + 0.5) if is_double[r] else (10 ** 6 + 17 * j, 10 ** 6 + 17 * j + 5)
    assert not np.any((m == 0) & (is_double[:, None] != 0))
    assert all(np.count_nonzero(m == v) == 1 for v in m[edge].ravel())
    a, b = m[:, 0].copy(), m[:, 1].copy()
    vals = np.choose(rs.randint(0, 5, R), [np.minimum(a, b) - 1, a, b, (a + b) / 2, np.maximum(a, b) + 1])
    assert np.all(vals[first:] != vals[:5]) and len(set(vals[edge].tolist())) == 6
    mean = (a + b) / 2.0
    da, db = a - mean, b - mean
    want = np.zeros((R, 8))
    want[:, 0] = mean
    want[:, 1] = np.sqrt((da * da + db * db) / 2.0)
    want[:, 2] = np.minimum(a, b)                                       # the wrapper's positions of two samples: 0 and 1
    want[:, 3] = np.maximum(a, b)
    want[:, 4] = (a < vals).astype(np.float64) + (b < vals)
    want[:, 5] = (a == vals).astype(np.float64) + (b == vals)
    return m, is_double, vals, want


def test_many_rows_reference_is_annotator_results():
    """no device: the vectorised expression of _many_rows is what AnnotatorResult computes row by row (a sample of rows here;
    the device test compares every row with the expression)"""
    m, is_double, vals, want = _many_rows()
    rows = list(range(40)) + list(range(FIRST_LAUNCH - 20, FIRST_LAUNCH + 5))
    assert {0, 1} == set(is_double[rows].tolist()) and len(set(want[rows, 4].tolist())) == 3
    for r in rows:
        h = gat_amd.AnnotatorResult("t", "a", "c", vals[r], m[r])
        d = gat_amd.AnnotatorResult("t", "a", "c", vals[r], m[r], _stats=tuple(want[r, :6]))
        assert (h.expected, h.stddev, h.lower95, h.upper95, h.pvalue) == (d.expected, d.stddev, d.lower95, d.upper95, d.pvalue)
        assert str(h) == str(d)


@gpu
def test_more_rows_than_one_launch(ctx):
    """2^20 + 5 rows: gat_null_stats' second launch and its four offset pointers; every slot of every row against numpy"""
    m, is_double, vals, want = _many_rows()
    slots = np.where(is_double[:, None] != 0, m.view(np.int64), m.astype(np.int64))
    dev = ctx.alloc(slots.nbytes)
    try:
        ctx.h2d(dev, slots)
        got = ctx.null_stats(dev, len(m), 2, is_double, vals)
    finally:
        ctx.free(dev)
    wrong = np.flatnonzero(np.any(got != want, axis=1))
    assert len(wrong) == 0, (len(wrong), wrong[:8].tolist(), got[wrong[:2]].tolist(), want[wrong[:2]].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# gat_minp_counts


def _device_counts(ctx, m, is_double, means, k_obs):
    slots = _slots(m, is_double)
    ptr = ctx.alloc(slots.nbytes)
    try:
        ctx.h2d(ptr, slots)
        return ctx.minp_counts(ptr, m.shape[0], m.shape[1], is_double, means, k_obs).tolist()
    finally:
        ctx.free(ptr)


_MODEL = {}


def _fuzz_family(R, S):
    """R rows drawn as test_minp_gpu.test_fuzz draws them (30 % doubles, widths of 1 to 100 000, a row repeating the one in
    front of it with probability 0.2) and the model's answer, computed once per shape"""
    key = ("fuzz", R, S)
    if key not in _MODEL:
        rs = np.random.RandomState(104729 * R + S)
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
        k_obs, c, _ = M.minp(m, means, obs)
        for a in (m, is_double):
            a.setflags(write=False)
        _MODEL[key] = (m, is_double, means, k_obs, c, _late_rows_that_matter(m, means, k_obs, c))
    return _MODEL[key]


def _late_rows_that_matter(m, means, k_obs, c):
    """of the rows behind the first 512 of the order k_minp_rank works in -- a workgroup's second and third -- how many get
    another count from the model when the running minimum leaves those rows out: what their K is worth to the comparison"""
    proc = sorted(range(len(m)), key=lambda r: (k_obs[r], r), reverse=True)
    q = np.full(m.shape[1], np.iinfo(np.int64).max, dtype=np.int64)
    for r in proc[:512]:
        q = np.minimum(q, M.t_row(m[r], means[r]))
    return sum(int(np.count_nonzero(q <= k_obs[r])) != c[r] for r in proc[512:])


def _family(R, S, first):
    key = (R, S, first)
    if key not in _MODEL:
        m, is_double, obs = M.family(np.random.RandomState(7919 * R + 31 * S + first), R, S, first)
        means = [float(np.mean(row)) for row in m]
        k_obs, c, _ = M.minp(m, means, obs)
        for a in (m, is_double):
            a.setflags(write=False)
        _MODEL[key] = (m, is_double, means, k_obs, c)
    return _MODEL[key]


def _rows_mb(n, S):
    """GAT_MINP_SCRATCH_MB for batches of n rows of K (half a row over, against the division's rounding)"""
    return repr((n + 0.5) * S * 4 / 1048576.0)


MINP_SORTS = ("lds", "lds 300", "global")
MINP_ROWS = [(R, sort, "default") for R in (513, 1025, 1100) for sort in MINP_SORTS] + [(1100, sort, "600 rows") for sort in MINP_SORTS]


def _minp_rows_case(R, sort):
    """the family of a case of test_minp_second_and_third_row_of_a_workgroup, with its premise: 65 samples are so few that
    the running minimum is 1 everywhere after 512 rows, and no count depends on a later row's K (those cases still run the
    loop and the carried q); at 300 samples and 1 025 rows or more, hundreds of counts do"""
    S = 65 if sort == "lds" else 300
    family = _fuzz_family(R, S)
    if S == 300 and R >= 1025:
        assert family[5] >= 500
    return S, family[:5]


@pytest.mark.parametrize("R,sort", sorted(set(c[:2] for c in MINP_ROWS)))
def test_minp_rows_premise_holds(R, sort):
    """no device"""
    _minp_rows_case(R, sort)


@gpu
@pytest.mark.parametrize("R,sort,scratch", MINP_ROWS)
def test_minp_second_and_third_row_of_a_workgroup(ctx, R, sort, scratch, monkeypatch):
    """more rows than k_minp_rank has workgroups (512): a workgroup sorts a second and a third row in the buffers of its
    first -- in LDS at 65 and at 300 samples, in global memory at 300 with GAT_MINP_LDS_SAMPLES=64; with 600 rows of K a
    batch, 1 100 rows are a batch of 600 on 512 workgroups and one of 500"""
    S, (m, is_double, means, k_obs, want) = _minp_rows_case(R, sort)
    if sort == "global":
        monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", "64")
    if scratch != "default":
        monkeypatch.setitem(ctx.options, "GAT_MINP_SCRATCH_MB", _rows_mb(600, S))
    # constant, double and repeated rows are among the workgroups' first rows (the order is (k_obs, index) from its end) and,
    # where there are 513 or more of them, among their later ones
    proc = sorted(range(R), key=lambda r: (k_obs[r], r), reverse=True)
    for part in (proc[:512], proc[512:]) if R >= 1025 else (proc[:512],):
        assert any(is_double[r] for r in part) and any(m[r].min() == m[r].max() for r in part)
        assert any(r > 0 and np.array_equal(m[r], m[r - 1]) for r in part)
    got = _device_counts(ctx, m, is_double, means, k_obs)
    wrong = [r for r in range(R) if got[r] != want[r]]
    assert not wrong, (len(wrong), [(r, proc.index(r), got[r], want[r]) for r in wrong[:8]])


def _lds_bound(ctx):
    """the largest GAT_MINP_LDS_SAMPLES, as the library's own message states it"""
    L = _lib.lib()
    slots = np.zeros((1, 1), dtype=np.int64)
    one = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    dbl, means, kobs, out = np.zeros(1, np.uint8), np.zeros(1), np.ones(1, np.int32), np.zeros(1, np.int64)
    ptr = ctx.alloc(slots.nbytes)
    ctx.options["GAT_MINP_LDS_SAMPLES"] = "1000000"
    try:
        ctx.h2d(ptr, slots)
        rc = L.gat_minp_counts(ctx._h, ctypes.c_void_p(ptr), 1, 1, one(dbl), one(means), one(kobs), one(out))
        text = L.gat_last_error(ctx._h).decode()
    finally:
        del ctx.options["GAT_MINP_LDS_SAMPLES"]
        ctx.free(ptr)
    assert rc == GAT_ERR_ARG
    found = re.search(r"must be in \[0, (\d+)\]", text)
    assert found, text
    return int(found.group(1))


def _check_families(ctx, R, S):
    for first in range(0, M.N_KINDS, R):
        m, is_double, means, k_obs, want = _family(R, S, first)
        got = _device_counts(ctx, m, is_double, means, k_obs)
        print("S=%d R=%d first=%d: k_obs=%s c=%s" % (S, R, first, k_obs[:8], got[:8]))
        assert got == want, (S, R, first)


@gpu
@pytest.mark.parametrize("S,R", [(4095, 7), (4096, 7), (4097, 7), (65537, 3), (100003, 3)])
def test_minp_large_rows_at_the_default_knobs(ctx, S, R):
    """the last rows sorted in LDS (16 keys a thread), the first on the global-memory path, and long ones on it: at 100 003
    samples a thread owns 391 keys and the last threads none"""
    assert "GAT_MINP_LDS_SAMPLES" not in ctx.options and ctx.options.get("GAT_MINP_LDS_SAMPLES") in (None, "4096")
    _check_families(ctx, R, S)


@gpu
def test_minp_all_passes_at_100003_samples(ctx, monkeypatch):
    monkeypatch.setitem(ctx.options, "GAT_MINP_ALL_PASSES", "1")
    _check_families(ctx, 3, 100003)


@gpu
@pytest.mark.parametrize("beyond", [0, 1])
def test_minp_largest_row_in_lds_and_the_first_beyond(ctx, beyond, monkeypatch):
    """GAT_MINP_LDS_SAMPLES at the largest value the library takes: a row of that many samples fills a workgroup's LDS, one
    sample more goes through global memory"""
    n = _lds_bound(ctx)
    assert n > 4097
    monkeypatch.setitem(ctx.options, "GAT_MINP_LDS_SAMPLES", str(n))
    _check_families(ctx, 7, n + beyond)
