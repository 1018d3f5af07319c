"""Python-int models of the deep null (gat_null_fold, gat_amd.run(null_round_size=...)): the eight words of a row from its
values, the sum of two rows' words, and a result row from its words.  Nothing here is floating point until the last two
divisions and the root; the device's words and the engine's rows have to equal these exactly."""
import math

WORDS = 8                     # n, sum, sumsq_lo, sumsq_hi, n_less, n_eq, min, max
M64 = (1 << 64) - 1
EMPTY = (0, 0, 0, 0, 0, 0, M64, 0)


def row_words(values, val):
    """the words of one row: `values` non-negative Python ints below 2^63, `val` the float the p-value is asked for.
    (Python compares an int with a float exactly.)"""
    values = [int(v) for v in values]
    assert all(0 <= v < (1 << 63) for v in values)
    sumsq = sum(v * v for v in values) & ((1 << 128) - 1)
    return (len(values), sum(values) & M64, sumsq & M64, sumsq >> 64,
            sum(1 for v in values if v < val), sum(1 for v in values if v == val),
            min(values) if values else M64, max(values) if values else 0)


def words(matrix, vals):
    """[row_words] of the rows of an integer matrix"""
    return [row_words([int(v) for v in row], float(val)) for row, val in zip(matrix, vals)]


def integer_parameters(val):
    """val as the two integers the library compares with: v < val is v < lt, v == val is v == eq (None: never)"""
    c = math.ceil(val)                                       # a Python int, exact
    lt = min(max(c, 0), 1 << 63)
    eq = c if (c == val and 0 <= c < (1 << 63)) else None
    return lt, eq


def words_numpy(matrix, vals):
    """words() for matrices too large for a Python loop, still exact: a value is cut into four 16-bit limbs, the ten limb
    products (below 2^32 each) are summed per row in uint64 (exact for fewer than 2^32 samples) and put together as Python
    ints; the two counts use integer_parameters.  tests/test_null_fold_model.py holds it against words()."""
    import numpy as np
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    n_rows, n = m.shape
    assert n < (1 << 32)
    limbs = [(m >> np.uint64(16 * i)) & np.uint64(0xFFFF) for i in range(4)]
    total = [sum(int(s) << (16 * i) for i, s in enumerate(per)) for per in zip(*[l.sum(axis=1, dtype=np.uint64).tolist() for l in limbs])]
    sumsq = [0] * n_rows
    for i in range(4):
        for j in range(i, 4):
            per = (limbs[i] * limbs[j]).sum(axis=1, dtype=np.uint64).tolist()
            for r in range(n_rows):
                sumsq[r] += (int(per[r]) * (1 if i == j else 2)) << (16 * (i + j))
    mn = m.min(axis=1).tolist() if n else [M64] * n_rows
    mx = m.max(axis=1).tolist() if n else [0] * n_rows
    out = []
    for r in range(n_rows):
        lt, eq = integer_parameters(float(vals[r]))
        less = int(np.count_nonzero(m[r] < np.uint64(lt))) if lt < (1 << 63) else n
        same = int(np.count_nonzero(m[r] == np.uint64(eq))) if eq is not None else 0
        sq = sumsq[r] & ((1 << 128) - 1)
        out.append((n, total[r] & M64, sq & M64, sq >> 64, less, same, int(mn[r]), int(mx[r])))
    return out


def add(a, b):
    """the words of two disjoint ranges of samples of one row"""
    sumsq = ((a[2] + (a[3] << 64)) + (b[2] + (b[3] << 64))) & ((1 << 128) - 1)
    return (a[0] + b[0], (a[1] + b[1]) & M64, sumsq & M64, sumsq >> 64, a[4] + b[4], a[5] + b[5], min(a[6], b[6]), max(a[7], b[7]))


def two_sided(n_less, n_eq, above_expected, n):
    """the reference's two-sided empirical p-value (a walk over the sorted samples there) from two counts"""
    idx = n_less
    if idx == n:
        idx = 1
    elif above_expected:
        if n_eq > 0 and idx > 0:
            idx -= 1
        idx = n - (idx + 1)
    else:
        idx += n_eq
    return max(1.0 / n, float(idx) / n)


def row(w, observed, fold=None, pseudo_count=1.0):
    """a result row from its words; fold: the reference row's fold change, if there is one (the words were then counted
    against observed / fold)"""
    n, total, sumsq = w[0], w[1], w[2] + (w[3] << 64)
    expected = total / n
    stddev = math.sqrt((n * sumsq - total * total) / (n * n))
    val = float(observed)
    if fold is not None:
        expected *= fold
        val = val / fold
    return dict(nsamples=n, expected=expected, stddev=stddev,
                fold=(float(observed) + pseudo_count) / (expected + pseudo_count) if expected != 0 else 1.0,
                pvalue=two_sided(w[4], w[5], val > expected, n))
