"""Model of --output-stats=segment_metrics / sample_metrics.  TEST INFRASTRUCTURE ONLY.

Two forms of the numbers behind SegmentsSummary.update (gat/IO.py:353-408):

  reference_lists / summary_attributes   the reference's three merge-joins restated in plain Python -- SegmentList.filter,
      intersect and subtract (gat/SegmentList.pyx:1401-1549, :1204-1285), statement by statement, with what they do at the
      ends of the lists: subtract's loop runs while BOTH lists have segments and then writes only the segment it holds, so
      the segments behind the last one that meets the intersection are missing from its result (all of them, where the
      intersection is empty: it then holds Segment(0, 0));
  words   the per-segment form the device computes (include/gat_mi355.h, gat_list_metrics): eight sums over the segments
      of a list, from two searches per segment.  It takes lists in any order.

For sorted, disjoint lists the two agree (tests/test_metrics_model.py); for other lists `words` is the definition.
"""
import bisect

WORDS = ("n", "bases", "pairs", "inter", "touched", "outside_pieces", "tail_n", "tail_bases")
INT_ATTRIBUTES = ("all_segments", "all_nucleotides", "segments_overlapping_workspace", "nucleotides_overlapping_workspace",
                  "segments_outside_workspace", "nucleotides_outside_workspace", "truncated_segments", "truncated_nucleotides")
FLOAT_ATTRIBUTES = ("density_workspace", "proportion_truncated_segments", "proportion_extending_nucleotides")


# ---- the reference's merge-joins ---------------------------------------------------------------------------------------------
def ref_filter(this, other):
    """SegmentList.filter: the segments of `this` that overlap a segment of `other`"""
    if not this:
        return []
    out = []
    ti = oi = 0
    last_start = this[0][0] - 1
    while ti < len(this) and oi < len(other):
        (ts, te), (os_, oe) = this[ti], other[oi]
        if te <= os_:
            ti += 1
        elif oe <= ts:
            oi += 1
        else:
            if last_start != ts:
                out.append((ts, te))
                last_start = ts
            if te < oe:
                ti += 1
            elif oe < te:
                oi += 1
            else:
                ti += 1
                oi += 1
    return out


def ref_intersect(this, other):
    """SegmentList.intersect: every overlap of a segment of `this` with a segment of `other`, not merged"""
    if not this:
        return []
    out = []
    ti = oi = 0
    while ti < len(this) and oi < len(other):
        (ts, te), (os_, oe) = this[ti], other[oi]
        if te <= os_:
            ti += 1
        elif oe <= ts:
            oi += 1
        else:
            out.append((max(ts, os_), min(te, oe)))
            if te < oe:
                ti += 1
            elif oe < te:
                oi += 1
            else:
                ti += 1
                oi += 1
    return out


def ref_subtract(this, other):
    """SegmentList.subtract as written: the loop ends with the shorter list, then `this_segment` -- the one segment held,
    Segment(0, 0) if the loop never ran -- is written if anything is left of it"""
    if not this:
        return []
    out = []
    ti = oi = 0
    last_ti = last_oi = -1
    ts = te = os_ = oe = 0
    while ti < len(this) and oi < len(other):
        if last_ti != ti:
            ts, te = this[ti]
            last_ti = ti
        if last_oi != oi:
            os_, oe = other[oi]
            last_oi = oi
        if te <= os_:
            if ts < te:
                out.append((ts, te))
            ti += 1
        elif oe <= ts:
            oi += 1
        else:
            if ts < os_:
                out.append((ts, os_))
            ts = oe
    if ts < te:
        out.append((ts, te))
    return out


def total(lst):
    return sum(e - s for s, e in lst)


def summary_attributes(segments, workspace):
    """SegmentsSummary.update(segments, workspace) for sorted, disjoint lists of (start, end): its attributes as a dict"""
    overlapping = ref_filter(segments, workspace)
    truncated = ref_intersect(overlapping, workspace)
    extending = ref_subtract(segments, truncated)
    a = dict(all_segments=len(segments), all_nucleotides=total(segments),
             segments_overlapping_workspace=len(truncated), nucleotides_overlapping_workspace=total(truncated),
             truncated_segments=len(extending), truncated_nucleotides=total(extending))
    a["segments_outside_workspace"] = a["all_segments"] - a["segments_overlapping_workspace"]
    a["nucleotides_outside_workspace"] = a["all_nucleotides"] - a["nucleotides_overlapping_workspace"]
    size = total(workspace)
    a["density_workspace"] = a["proportion_truncated_segments"] = a["proportion_extending_nucleotides"] = 0.0
    if size > 0:
        a["density_workspace"] = float(a["nucleotides_overlapping_workspace"]) / size
    if a["segments_overlapping_workspace"] > 0:
        a["proportion_truncated_segments"] = float(a["truncated_segments"]) / a["segments_overlapping_workspace"]
        a["proportion_extending_nucleotides"] = float(a["truncated_nucleotides"]) / total(overlapping)
    a["_touched"] = total(overlapping)
    return a


# ---- the per-segment form ----------------------------------------------------------------------------------------------------
def words(segments, workspace):
    """the eight sums of a list of (start, end) in any order against normalized pieces (sorted, disjoint, maybe adjacent)"""
    starts = [w[0] for w in workspace]
    ends = [w[1] for w in workspace]
    cum = [0]
    gaps = [0]
    for j, (ws, we) in enumerate(workspace):
        cum.append(cum[-1] + we - ws)
        if j > 0:
            gaps.append(gaps[-1] + (1 if ws > workspace[j - 1][1] else 0))
    n = bases = pairs = inter = touched = pieces = 0
    last = -1
    for s, e in segments:
        n += 1
        bases += e - s
        lo = bisect.bisect_right(ends, s)                 # the first piece with end > s
        hi = bisect.bisect_left(starts, e) - 1            # the last piece with start < e
        k = max(0, hi - lo + 1)
        if k == 0:
            pieces += 1
            continue
        last = max(last, s)
        pairs += k
        touched += e - s
        inter += cum[hi + 1] - cum[lo] - max(0, s - starts[lo]) - max(0, ends[hi] - e)
        pieces += (1 if s < starts[lo] else 0) + (1 if e > ends[hi] else 0) + gaps[hi] - gaps[lo]
    tail = [(s, e) for s, e in segments if s > last]
    return [n, bases, pairs, inter, touched, pieces, len(tail), total(tail)]


def attributes_from_words(w, workspace_bases):
    """the reference's attributes from the eight sums"""
    n, bases, pairs, inter, touched, pieces, tail_n, tail_bases = w
    a = dict(all_segments=n, all_nucleotides=bases, segments_overlapping_workspace=pairs, nucleotides_overlapping_workspace=inter,
             segments_outside_workspace=n - pairs, nucleotides_outside_workspace=bases - inter,
             truncated_segments=pieces - tail_n, truncated_nucleotides=bases - inter - tail_bases, _touched=touched)
    a["density_workspace"] = float(inter) / workspace_bases if workspace_bases > 0 else 0.0
    a["proportion_truncated_segments"] = float(a["truncated_segments"]) / pairs if pairs > 0 else 0.0
    a["proportion_extending_nucleotides"] = float(a["truncated_nucleotides"]) / touched if pairs > 0 else 0.0
    return a


def words_of_array(a, w):
    """words() on SEG arrays"""
    return words(list(zip(a["start"].tolist(), a["end"].tolist())), list(zip(w["start"].tolist(), w["end"].tolist())))
