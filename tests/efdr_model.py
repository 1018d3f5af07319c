"""The numpy model of the resampling-based false discovery rate (--qvalue-method=efdr, --output-stats=fdr_summary) as gat_amd
computes it, written from the definitions and sharing nothing with gat_amd/efdr.py.

A family is R rows of S samples; T, k_obs[r] = T(r, observed_r) and K[r][i] = T(r, row_r[i]) are those of minp_model.py
(pvalue = T / S).  In addition

    D[r][i]  = 1 if row_r[i] > e_r else 0            (the comparison T branches on: 1 = the over-represented tail)
    Dobs[r]  = 1 if observed_r > e_r else 0
    V_d(t)   = #{(r, i) : K[r][i] <= t and D[r][i] == d},  d in {1, 0};  V(t) = V_1(t) + V_0(t)
    Rn(t)    = #{r : k_obs[r] <= t}
    fdr(t)   = V(t) / (S * Rn(t))
    o_1..o_R = the rows by (k_obs, row index) ascending
    q[o_j]   = min(1.0, max(1.0 / S, min over j' >= j of fdr(k_obs[o_j'])))

and for a cutoff p, with the level L = int(p * S) and N_d[i] = #{r : K[r][i] <= L and D[r][i] == d}: observed significant
= #{r : k_obs[r] <= L}, over = those with Dobs == 1, under = the rest; per category (significant: N_1 + N_0, over: N_1,
under: N_0), with s the S values sorted ascending, average = sum / S ("%.2f"), median = s[S // 2], limit95 = s[(19 * S) // 20];
"na" for the three when L == 0.
"""
import numpy as np

from minp_model import family, k_obs_of, order, t_row  # noqa: F401  (family, k_obs_of: for the tests that import this module)

HEADER = "pvalue_cutoff\tlevel\tcategory\tobserved\taverage\tmedian\tlimit95"


def _k_and_d(matrix, expected):
    K = np.stack([t_row(row, e) for row, e in zip(matrix, expected)])
    D = np.stack([np.asarray(row, dtype=np.float64) > e for row, e in zip(matrix, expected)])
    return K, D


def v_at(matrix, expected, t):
    """(V_1(t), V_0(t))"""
    K, D = _k_and_d(matrix, expected)
    return int(np.count_nonzero((K <= t) & D)), int(np.count_nonzero((K <= t) & ~D))


def counts(matrix, expected, k_obs):
    """[R][2]: V_1(k_obs[r]), V_0(k_obs[r]), in the order of the rows"""
    K, D = _k_and_d(matrix, expected)
    return [[int(np.count_nonzero((K <= t) & D)), int(np.count_nonzero((K <= t) & ~D))] for t in k_obs]


def per_sample(matrix, expected, levels):
    """[n_levels][2][S]: N_1, N_0 per level"""
    K, D = _k_and_d(matrix, expected)
    out = np.zeros((len(levels), 2, K.shape[1]), dtype=np.int64)
    for l, L in enumerate(levels):  # noqa: E741
        out[l, 0] = np.count_nonzero((K <= L) & D, axis=0)
        out[l, 1] = np.count_nonzero((K <= L) & ~D, axis=0)
    return out


def adjusted(k_obs, v, S):
    """q in the order of the rows, from v = counts(...)"""
    o = order(k_obs)
    fdr = []
    for r in o:
        rn = sum(1 for k in k_obs if k <= k_obs[r])
        fdr.append((v[r][0] + v[r][1]) / (S * rn))
    out = [None] * len(k_obs)
    for j, r in enumerate(o):
        out[r] = min(1.0, max(1.0 / S, min(fdr[j:])))
    return out


def efdr(matrix, expected, observed):
    """(k_obs, v, q), each in the order of the rows"""
    k_obs = k_obs_of(matrix, expected, observed)
    v = counts(matrix, expected, k_obs)
    return k_obs, v, adjusted(k_obs, v, len(matrix[0]))


def summary(matrix, expected, observed, pvalue_cutoffs):
    """rows (pvalue_cutoff, level, category, observed, average, median, limit95), three per cutoff; the last three are the
    strings of the file"""
    S = len(matrix[0])
    k_obs = k_obs_of(matrix, expected, observed)
    levels = [int(p * S) for p in pvalue_cutoffs]
    N = per_sample(matrix, expected, levels)
    rows = []
    for p, L, n in zip(pvalue_cutoffs, levels, N):
        sig = [r for r in range(len(k_obs)) if k_obs[r] <= L]
        over = [r for r in sig if observed[r] > expected[r]]
        for category, obs, values in (("significant", len(sig), n[0] + n[1]), ("over", len(over), n[0]),
                                      ("under", len(sig) - len(over), n[1])):
            if L == 0:
                rows.append((p, L, category, obs, "na", "na", "na"))
            else:
                s = sorted(int(x) for x in values)
                rows.append((p, L, category, obs, "%.2f" % (sum(s) / S), "%i" % s[S // 2], "%i" % s[(19 * S) // 20]))
    return rows


def format_summary(rows):
    lines = [HEADER]
    for p, L, category, obs, average, median, limit in rows:
        lines.append("\t".join(("%g" % p, "%i" % L, category, "%i" % obs, average, median, limit)))
    return "\n".join(lines) + "\n"
