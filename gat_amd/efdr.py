"""--qvalue-method=efdr and --output-stats=fdr_summary: the resampling-based false discovery rate, the FDR counterpart of
step-down minP (gat_amd/minp.py) and what the Annotator's "False Discovery summary" estimates
(annotator/src/app/FalseDiscoveryStats.java; Engine.computeFDR, gat/Engine.pyx:3366-3501, is its obsolete port).

Column i of the count matrix of a run is one draw from the joint null distribution of the whole result table, so the number of
rows of column i that would be called at a threshold is one draw of the number of false calls there.  With T, k_obs and
K[r][i] = T(r, row_r[i]) those of minp.py (pvalue = T / S):

    D[r][i]  = 1 if row_r[i] > expected_r else 0      (the comparison T branches on: 1 = the over-represented tail)
    V_d(t)   = #{(r, i) : K[r][i] <= t and D[r][i] == d},   V(t) = V_1(t) + V_0(t)
    Rn(t)    = #{r : k_obs[r] <= t}
    fdr(t)   = V(t) / (S * Rn(t))
    o_1..o_R   the rows by (k_obs, index) ascending
    q[o_j]   = min(1, max(1 / S, min over j' >= j of fdr(k_obs[o_j'])))

T is the one-tailed p-value in the observed direction: on one calibrated row V(t) is about 2 t and q about 2 p, which is why
the summary reports the two directions apart.  The false discovery summary of a cutoff p, with L = int(p * S) (the Annotator's
level) and N_d[i] = #{r : K[r][i] <= L and D[r][i] == d}: the observed number of rows at or below L -- all of them, those
above their expected value, the rest -- beside the average, the median (s[S // 2]) and the 95 % limit (s[(19 * S) // 20]) of
N_1 + N_0, N_1 and N_0 over the samples.  L == 0: "na", the Annotator's "insufficiently many samples".  pi0 is taken as 1.

V and N are formed on the device (gat_efdr_counts: k_minp_rank + k_efdr, DESIGN.md section 5 "k_efdr"); the order, Rn, the
running minimum, the division and the order statistics of N are the host's, here.  There is no CPU path.
"""
import numpy as np

from . import minp

MAX_LEVELS = 8                      # levels of one gat_efdr_counts call
SUMMARY_HEADER = "pvalue_cutoff\tlevel\tcategory\tobserved\taverage\tmedian\tlimit95"
CATEGORIES = ("significant", "over", "under")


def adjusted(k_obs, v, nsamples):
    """the q-values, in the order of the rows, from the device's counts v[r] = (V_1, V_0) at k_obs[r]: walking o_R .. o_1, Rn
    is the number of rows up to the last one tied with the row, and q the running minimum of V / (S * Rn), kept within
    [1 / S, 1]"""
    o = minp.order(k_obs)
    out = [1.0] * len(k_obs)
    run = None
    rn = 0
    for j in range(len(o) - 1, -1, -1):
        r = o[j]
        if j == len(o) - 1 or k_obs[o[j + 1]] != k_obs[r]:
            rn = j + 1
        fdr = (int(v[r][0]) + int(v[r][1])) / (nsamples * rn)
        run = fdr if run is None else min(run, fdr)
        out[r] = min(1.0, max(1.0 / nsamples, run))
    return out


def level_of(pvalue_cutoff, nsamples):
    return int(pvalue_cutoff * nsamples)


def _statistics(n, nsamples):
    s = np.sort(np.asarray(n, dtype=np.int64))
    return "%.2f" % (int(s.sum()) / nsamples), "%i" % s[nsamples // 2], "%i" % s[(19 * nsamples) // 20]


def summarise(k_obs, d_obs, per_sample, pvalue_cutoffs, nsamples):
    """the summary rows (pvalue_cutoff, level, category, observed, average, median, limit95) -- the last three as the strings
    the file holds -- from per_sample[c] = (N_1, N_0) at the level of pvalue_cutoffs[c]; d_obs[r]: observed_r > expected_r"""
    rows = []
    for c, p in enumerate(pvalue_cutoffs):
        L = level_of(p, nsamples)
        called = [r for r in range(len(k_obs)) if k_obs[r] <= L]
        over = sum(1 for r in called if d_obs[r])
        n1, n0 = (np.asarray(x, dtype=np.int64) for x in per_sample[c])
        for category, observed, n in zip(CATEGORIES, (len(called), over, len(called) - over), (n1 + n0, n1, n0)):
            rows.append((p, L, category, observed) + (_statistics(n, nsamples) if L > 0 else ("na", "na", "na")))
    return rows


def format_summary(rows):
    return "".join([SUMMARY_HEADER + "\n"] + ["%g\t%i\t%s\t%i\t%s\t%s\t%s\n" % tuple(r) for r in rows])


def compute(results, pvalue_cutoffs=(), ctx=None):
    """(q-values in the order of `results`, summary rows for `pvalue_cutoffs`) of a list of AnnotatorResult -- the rows of one
    outputResults call -- from ONE upload of their samples (a float64 matrix, every row flagged double) and one gat_efdr_counts
    call per 8 cutoffs.  ValueError as minp.adjust raises them: rows of different nsamples, a row without samples, a row built
    with a `reference`."""
    results = list(results)
    pvalue_cutoffs = list(pvalue_cutoffs)
    if not results:
        return [], []
    nsamples, k_obs, means, m = minp._rows(results, method="efdr")
    for p in pvalue_cutoffs:
        if not 0.0 <= p <= 1.0:
            raise ValueError("fdr summary: p-value cutoff %r is outside [0, 1]" % (p,))
    levels = [level_of(p, nsamples) for p in pvalue_cutoffs]
    if ctx is None:
        from .engine import get_context
        ctx = get_context()
    ones = np.ones(m.shape[0], dtype=np.uint8)
    ptr = ctx.alloc(m.nbytes)
    try:
        ctx.h2d(ptr, m)
        v, per_sample = ctx.efdr_counts(ptr, m.shape[0], nsamples, ones, means, k_obs, levels[:MAX_LEVELS])
        for first in range(MAX_LEVELS, len(levels), MAX_LEVELS):
            per_sample = np.concatenate((per_sample, ctx.efdr_counts(ptr, m.shape[0], nsamples, ones, means, k_obs,
                                                                     levels[first:first + MAX_LEVELS])[1]))
    finally:
        ctx.free(ptr)
    d_obs = [x.observed > x.expected for x in results]
    return adjusted(k_obs, v, nsamples), summarise(k_obs, d_obs, per_sample, pvalue_cutoffs, nsamples)


def adjust(results, ctx=None):
    """the q-values of `results`, in their order (compute without a summary)"""
    return compute(results, (), ctx=ctx)[0]


def summary(results, pvalue_cutoffs, ctx=None):
    """the false discovery summary rows of `results` for `pvalue_cutoffs` (compute without the q-values)"""
    return compute(results, pvalue_cutoffs, ctx=ctx)[1]
