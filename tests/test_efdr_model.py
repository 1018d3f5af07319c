"""CPU: the numpy model of the resampling-based FDR (tests/efdr_model.py) against a literal double loop over (r, i), its
invariants, and the statistical statement it is used for: shifted rows of a family of independent rows are found, null rows
are not."""
import numpy as np
import pytest

import efdr_model as E
import minp_model as M


def _literal(matrix, expected, observed, levels):
    """V at every k_obs and N at every level by a double loop over (r, i), T by its definition (minp_model.t_value)"""
    R, S = len(matrix), len(matrix[0])
    k_obs = [M.t_value(matrix[r], expected[r], observed[r]) for r in range(R)]
    v = [[0, 0] for _ in range(R)]
    n = [[[0] * S, [0] * S] for _ in levels]
    for r in range(R):
        for i in range(S):
            k = M.t_value(matrix[r], expected[r], matrix[r][i])
            d = 1 if matrix[r][i] > expected[r] else 0
            for rr in range(R):
                if k <= k_obs[rr]:
                    v[rr][1 - d] += 1
            for l, L in enumerate(levels):  # noqa: E741
                if k <= L:
                    n[l][1 - d][i] += 1
    return k_obs, v, n


def _families():
    for R, S in ((1, 1), (1, 2), (2, 5), (3, 64), (7, 65), (6, 33)):
        for first in (range(0, M.N_KINDS, R) if R < M.N_KINDS else [0]):
            m, _, obs = M.family(np.random.RandomState(100 * R + S + first), R, S, first)
            yield m, [float(np.mean(row)) for row in m], obs


def test_model_equals_the_literal_double_loop():
    n = 0
    for m, means, obs in _families():
        S = m.shape[1]
        levels = [0, 1, int(0.05 * S), S // 2, S]
        k_obs, v, per = _literal(m, means, obs, levels)
        assert k_obs == M.k_obs_of(m, means, obs)
        assert E.counts(m, means, k_obs) == v
        assert E.per_sample(m, means, levels).tolist() == per
        n += 1
    assert n >= 10


def test_per_sample_sums_to_v_and_v_is_monotone_and_complete():
    for m, means, obs in _families():
        R, S = m.shape
        levels = list(range(0, S + 1))
        per = E.per_sample(m, means, levels)
        last = (0, 0)
        for L in levels:
            v = E.v_at(m, means, L)
            assert (int(per[L][0].sum()), int(per[L][1].sum())) == v
            assert v[0] >= last[0] and v[1] >= last[1]
            last = v
        assert per[0].sum() == 0                                   # K >= 1
        assert sum(E.v_at(m, means, S)) == R * S


def test_q_is_monotone_along_the_order_and_bounded():
    for m, means, obs in _families():
        S = m.shape[1]
        k_obs, v, q = E.efdr(m, means, obs)
        o = M.order(k_obs)
        assert all(q[o[j]] <= q[o[j + 1]] for j in range(len(o) - 1))
        assert all(1.0 / S <= x <= 1.0 for x in q)


def test_rn_counts_tied_rows_and_the_floor():
    # two rows with the same k_obs share Rn = 2; V = 0 gives the floor 1 / S
    assert E.adjusted([3, 3, 10], [[2, 1], [2, 1], [20, 10]], 10) == [3 / 20, 3 / 20, 1.0]
    assert E.adjusted([1], [[0, 0]], 4) == [0.25]
    # the running minimum: a later, smaller fdr pulls the earlier rows down
    assert E.adjusted([2, 5], [[6, 0], [4, 4]], 10) == [0.4, 0.4]


def test_summary_statistics_and_na():
    m, _, obs = M.family(np.random.RandomState(5), 7, 65, 0)
    means = [float(np.mean(row)) for row in m]
    rows = E.summary(m, means, obs, [0.0, 0.01, 0.05, 1.0])
    assert [r[1] for r in rows] == [0] * 6 + [3] * 3 + [65] * 3
    assert all(r[4:] == ("na", "na", "na") for r in rows[:6]) and all(r[3] == 0 for r in rows[:6])
    assert [r[2] for r in rows[:3]] == ["significant", "over", "under"]
    sig, over, under = rows[9:12]                                  # L = S: every row, every sample
    assert sig[3] == 7 and over[3] + under[3] == 7
    assert sig[4:] == ("7.00", "7", "7")
    text = E.format_summary(rows)
    assert text.splitlines()[0] == E.HEADER and len(text.splitlines()) == 13
    assert text.splitlines()[7].split("\t")[:3] == ["0.05", "3", "significant"]


@pytest.fixture(scope="module")
def poisson_family():
    rs = np.random.RandomState(1)
    m = rs.poisson(50, (200, 2000)).astype(np.float64)
    obs = rs.poisson(50, 200).astype(np.float64)
    obs[:10] += 40
    return m, [float(np.mean(row)) for row in m], obs


def test_shifted_rows_of_an_independent_family_are_found(poisson_family):
    m, means, obs = poisson_family
    _, _, q = E.efdr(m, means, obs)
    print("smallest null q-value: %.3f; largest shifted: %.4f" % (min(q[10:]), max(q[:10])))
    assert [r for r in range(200) if q[r] < 0.05] == list(range(10))
