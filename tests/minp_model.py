"""The numpy model of step-down minP (Westfall and Young; Ge, Dudoit and Speed 2003) as gat_amd computes it on the device,
written from the definition -- a loop over j -- and sharing nothing with gat_amd/minp.py.

A family is R rows of S samples; row r has its samples row_r, its expected value e_r (the numpy mean AnnotatorResult holds)
and its observed value obs_r.  T(r, x) is the integer AnnotatorResult._two_sided turns into a p-value:

    n_less = #{i : row_r[i] < x},  n_eq = #{i : row_r[i] == x}
    idx = 1                                             if n_less == S
        = S - (n_less - [n_eq > 0 and n_less > 0] + 1)  if x > e_r
        = n_less + n_eq                                 otherwise
    T = max(1, idx)                                     pvalue = T / S
"""
import numpy as np


def t_value(row, expected, x):
    row = np.asarray(row, dtype=np.float64)
    S = len(row)
    n_less = int(np.count_nonzero(row < x))
    n_eq = int(np.count_nonzero(row == x))
    if n_less == S:
        idx = 1
    elif x > expected:
        idx = S - (n_less - (1 if (n_eq > 0 and n_less > 0) else 0) + 1)
    else:
        idx = n_less + n_eq
    return max(1, idx)


def t_row(row, expected):
    """K[r][i] = T(r, row_r[i]) for every sample of the row: t_value vectorised over x (sort + two searches)"""
    row = np.asarray(row, dtype=np.float64)
    S = len(row)
    s = np.sort(row)
    n_less = np.searchsorted(s, row, side="left")
    n_eq = np.searchsorted(s, row, side="right") - n_less
    idx = np.where(row > expected, S - (n_less - ((n_eq > 0) & (n_less > 0)) + 1), n_less + n_eq)
    idx = np.where(n_less == S, 1, idx)
    return np.maximum(1, idx).astype(np.int64)


def k_obs_of(matrix, expected, observed):
    return [t_value(row, e, o) for row, e, o in zip(matrix, expected, observed)]


def order(k_obs):
    """o_1 .. o_R: the rows by (k_obs, row index) ascending"""
    return sorted(range(len(k_obs)), key=lambda r: (k_obs[r], r))


def counts(matrix, expected, k_obs):
    """c[r] = #{i : q_j[i] <= k_obs[o_j]} for r = o_j, in the order of the rows -- before the running maximum"""
    R = len(matrix)
    S = len(matrix[0])
    o = order(k_obs)
    q = np.full(S, np.iinfo(np.int64).max, dtype=np.int64)         # q_{R+1} = +inf
    c = [0] * R
    for j in range(R - 1, -1, -1):
        r = o[j]
        q = np.minimum(q, t_row(matrix[r], expected[r]))
        c[r] = int(np.count_nonzero(q <= k_obs[r]))
    return c


def adjusted(k_obs, c, S):
    """the adjusted p-value of o_j: the largest of max(1, c[o_j']) / S over j' <= j; in the order of the rows"""
    out = [None] * len(k_obs)
    run = 0
    for r in order(k_obs):
        run = max(run, max(1, c[r]))
        out[r] = float(run) / S
    return out


def minp(matrix, expected, observed):
    """(k_obs, c, adjusted p-values), each in the order of the rows"""
    k_obs = k_obs_of(matrix, expected, observed)
    c = counts(matrix, expected, k_obs)
    return k_obs, c, adjusted(k_obs, c, len(matrix[0]))


N_KINDS = 6


def family(rs, R, S, first=0):
    """The matrix contents the GPU tests use for a shape (float64 rows, a flag per row: held as int64 or as double on the
    device) and the observed values.  Row r is of kind first + r: kind 0 three distinct values (long ties), kind 1 constant
    with the observed value ON the constant (k_obs = S), kind 2 constant with the observed value off it (k_obs = 1, c = 0),
    kind 3 doubles with negative values and values below 1, kinds 4 and 5 the same row and observed value (equal k_obs: the
    order falls back to the index); beyond that random counts, with observed values below, inside and above the sampled
    range in turn.  A family of fewer than N_KINDS rows is drawn once per `first` in range(0, N_KINDS, R), so that every
    kind is met at every shape."""
    m = np.zeros((R, S), dtype=np.float64)
    is_double = np.zeros(R, dtype=np.uint8)
    obs = np.zeros(R, dtype=np.float64)
    for r in range(R):
        kind = min(first + r, N_KINDS)
        if kind == 5 and r == 0:
            kind = 4
        if kind == 0:
            m[r] = rs.choice([300.0, 301.0, 305.0], S)
            obs[r] = 301.0
        elif kind == 1:
            m[r] = 777.0
            obs[r] = 777.0
        elif kind == 2:
            m[r] = 12.0
            obs[r] = 13.0
        elif kind == 3:
            m[r] = np.round(rs.normal(0.0, 1.5, S), 3)
            m[r][rs.randint(0, S)] = -0.0
            is_double[r] = 1
            obs[r] = 0.25
        elif kind == 4:
            m[r] = rs.randint(50, 60, S)
            obs[r] = 57.0
        elif kind == 5:
            m[r] = m[r - 1]
            obs[r] = obs[r - 1]
        else:
            lo = int(rs.randint(0, 5000))
            m[r] = rs.randint(lo, lo + int(rs.choice([3, 40, 4000])), S)
            where = r % 4
            obs[r] = (m[r].min() - 3, float(np.median(m[r])), m[r].max() + 2, m[r].max())[where]
    return m, is_double, obs
