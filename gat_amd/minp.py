"""--qvalue-method=minp: Westfall and Young's step-down minP adjusted p-values (in the formulation of Ge, Dudoit and Speed
2003, "Resampling-based multiple testing for microarray data analysis"), read off the samples a run already holds.

Column i of the count matrix of a run is what EVERY annotation scored on the same sampled segment list: the rows of one
result table share their null samples, so the matrix is a sample of the joint null distribution of the whole family,
whatever the dependence between the annotations.  With T(r, x) the integer AnnotatorResult._two_sided turns into a p-value
(pvalue = T / S) and k_obs[r] = T(r, observed_r):

    K[r][i] = T(r, row_r[i])                          every sample scored against its own row
    o_1 .. o_R                                        the rows by (k_obs, index) ascending
    q_j[i]  = min(q_{j+1}[i], K[o_j][i])              from j = R down, q_{R+1} = +inf
    c[o_j]  = #{i : q_j[i] <= k_obs[o_j]}
    adjusted(o_j) = max over j' <= j of max(1, c[o_j']) / S

K, q and c are formed on the device (gat_minp_counts: k_minp_rank + k_minp_step, DESIGN.md section 5 "k_minp"); the order,
the running maximum and the division are the host's, here.  There is no CPU path.
"""
import numpy as np


def order(k_obs):
    """o_1 .. o_R: the rows by (k_obs, row index) ascending"""
    return sorted(range(len(k_obs)), key=lambda r: (k_obs[r], r))


def adjusted(k_obs, c, nsamples):
    """the adjusted p-values, in the order of the rows, from the device's counts: the running maximum of max(1, c) / S
    along o_1 .. o_R (max(1, .): the reference's min_pval floor)"""
    out = [1.0] * len(k_obs)
    run = 0
    for r in order(k_obs):
        run = max(run, 1, int(c[r]))
        out[r] = float(run) / nsamples
    return out


def _rows(results, method="minp"):
    """(nsamples, k_obs, means, the float64 matrix) of a list of AnnotatorResult; ValueError where the procedure does not
    apply (`method`: the name the message gives it; gat_amd/efdr.py reads its rows here too)"""
    nsamples = None
    k_obs, means, rows = [], [], []
    for x in results:
        if not hasattr(x, "_two_sided") or not hasattr(x, "samples"):
            raise ValueError("qvalue method %s: row (%s, %s) holds no samples (a results table read back has none; start "
                             "from the run or from its counts file)" % (method, getattr(x, "track", "?"), getattr(x, "annotation", "?")))
        if getattr(x, "_has_reference", False):
            raise ValueError("qvalue method %s: row (%s, %s) was built with a reference: its expected value is not the "
                             "mean of its samples" % (method, x.track, x.annotation))
        if nsamples is None:
            nsamples = x.nsamples
        elif x.nsamples != nsamples:
            raise ValueError("qvalue method %s: rows of %d and %d samples (one family shares its samples)" % (method, nsamples, x.nsamples))
        k_obs.append(int(round(x._two_sided(x.observed) * x.nsamples)))
        means.append(x.expected)
        rows.append(x.samples)
    return nsamples, k_obs, means, np.ascontiguousarray(np.stack(rows), dtype=np.float64)


def adjust(results, ctx=None):
    """The step-down minP adjusted p-values of `results` (a list of AnnotatorResult: the rows of one outputResults call), in
    their order.  The rows' samples go to the device as one float64 matrix (counts are exact in a double), every row flagged
    double.  ValueError: rows of different nsamples, a row without samples, a row built with a `reference`."""
    results = list(results)
    if not results:
        return []
    nsamples, k_obs, means, m = _rows(results)
    if ctx is None:
        from .engine import get_context
        ctx = get_context()
    ptr = ctx.alloc(m.nbytes)
    try:
        ctx.h2d(ptr, m)
        c = ctx.minp_counts(ptr, m.shape[0], nsamples, np.ones(m.shape[0], dtype=np.uint8), means, k_obs)
    finally:
        ctx.free(ptr)
    return adjusted(k_obs, c, nsamples)
