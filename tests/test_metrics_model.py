"""CPU: the model of the metrics (tests/metrics_model.py) against the reference's own numbers (tests/golden/metrics/kat.json,
made by tests/golden/make_metrics_goldens.py), its two forms against each other on fuzzed lists, and the Summary text of
gat_amd/metrics.py against the rows the reference's outputMetrics wrote."""
import io
import json
import os
import random

import numpy as np
import pytest

import metrics_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "metrics")
TOP = 2 ** 31 - 1


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLD, "kat.json")))


def _lists(case):
    return [tuple(x) for x in case["segments"]], [tuple(x) for x in case["workspace"]]


def test_merge_joins_equal_the_reference(kat):
    assert len(kat["cases"]) >= 30
    for case in kat["cases"]:
        got = M.summary_attributes(*_lists(case))
        for a in M.INT_ATTRIBUTES + M.FLOAT_ATTRIBUTES:
            assert got[a] == case[a], (case["name"], a, got[a], case[a])


def test_per_segment_form_equals_the_reference(kat):
    for case in kat["cases"]:
        segs, ws = _lists(case)
        got = M.attributes_from_words(M.words(segs, ws), M.total(ws))
        for a in M.INT_ATTRIBUTES + M.FLOAT_ATTRIBUTES:
            assert got[a] == case[a], (case["name"], a, got[a], case[a])


def test_kat_geometry(kat):
    """the cases hold what they are there for"""
    by = dict((c["name"], c) for c in kat["cases"])
    assert by["after_last"]["truncated_segments"] == 0 and by["after_last"]["nucleotides_outside_workspace"] == 1010    # subtract's end
    assert by["empty_workspace"]["truncated_nucleotides"] == 0 and by["empty_workspace"]["nucleotides_outside_workspace"] == 20
    assert by["over_two_adjacent"]["segments_overlapping_workspace"] == 2 and by["over_two_adjacent"]["truncated_segments"] == 0
    assert by["over_two_with_gap"]["truncated_segments"] == 1
    assert by["over_all_pieces"]["truncated_segments"] == 3
    assert max(e for c in kat["cases"] for _, e in c["segments"]) == TOP


def fuzz_list(r, n, top, p_adjacent, maxlen, maxgap):
    """a sorted, disjoint list of at most n segments below `top`; a neighbour is adjacent with probability p_adjacent"""
    out, pos = [], r.randint(0, maxgap)
    for _ in range(n):
        ln = r.randint(1, maxlen)
        if pos + ln > top:
            break
        out.append((pos, pos + ln))
        pos += ln + (0 if r.random() < p_adjacent else r.randint(1, maxgap))
    return out


def fuzz_cases(count=3000, seed=20261018):
    r = random.Random(seed)
    for i in range(count):
        n_s, n_w = r.choice([0, 1, 2, 5, 30, 120]), r.choice([0, 1, 2, 3, 8, 40, 150])
        scale = r.choice([1, 1, 10, 1000])
        segs = fuzz_list(r, n_s, TOP, r.choice([0.15, 0.5]), r.choice([1, 4, 50]) * scale, r.choice([2, 30, 300]) * scale)
        ws = fuzz_list(r, n_w, TOP, r.choice([0.15, 0.5]), r.choice([1, 6, 80]) * scale, r.choice([2, 20, 500]) * scale)
        if i % 7 == 0:                                   # pushed up against 2^31 - 1
            top = max([e for _, e in segs + ws] or [0])
            d = TOP - top
            if i % 14 == 0 and segs and ws:              # ... one of the two alone: the other then lies far below
                segs = [(s + d + top - segs[-1][1], e + d + top - segs[-1][1]) for s, e in segs]
            else:
                segs, ws = [(s + d, e + d) for s, e in segs], [(s + d, e + d) for s, e in ws]
        yield segs, ws


def test_two_forms_agree_on_fuzzed_lists():
    pairs_s = adj_s = pairs_w = adj_w = empty_s = empty_w = at_top = tails = 0
    for segs, ws in fuzz_cases():
        for lst in (segs, ws):
            assert all(s < e for s, e in lst) and all(lst[j][1] <= lst[j + 1][0] for j in range(len(lst) - 1))
        pairs_s += max(0, len(segs) - 1)
        adj_s += sum(segs[j][1] == segs[j + 1][0] for j in range(len(segs) - 1))
        pairs_w += max(0, len(ws) - 1)
        adj_w += sum(ws[j][1] == ws[j + 1][0] for j in range(len(ws) - 1))
        empty_s += not segs
        empty_w += not ws
        at_top += bool(segs + ws) and max(e for _, e in segs + ws) == TOP
        want = M.summary_attributes(segs, ws)
        w = M.words(segs, ws)
        tails += w[6] > 0 and w[2] > 0
        got = M.attributes_from_words(w, M.total(ws))
        assert got == want, (segs, ws, got, want)
    # the fuzz reaches what it is meant to reach
    assert adj_s * 10 >= pairs_s > 10000 and adj_w * 10 >= pairs_w > 10000, (adj_s, pairs_s, adj_w, pairs_w)
    assert empty_s > 100 and empty_w > 100 and at_top > 300 and tails > 100, (empty_s, empty_w, at_top, tails)


def test_summary_text_equals_the_golden_rows(kat):
    """gat_amd.metrics.write_rows over the model's sums writes what the reference's outputMetrics wrote"""
    from gat_amd import metrics
    by = dict((c["name"], c) for c in kat["cases"])
    assert any(len(g["keys"]) == 0 for g in kat["groups"]) and any(len(g["keys"]) > 20 for g in kat["groups"])
    for i, g in enumerate(kat["groups"]):
        cases = [by[k] for k in g["keys"]]
        words = np.array([M.words(*_lists(c)) for c in cases], dtype=np.int64).reshape(1, len(cases), len(M.WORDS))
        out = io.StringIO()
        metrics.write_rows(out, "kat", ["group%d" % i], words, [M.total(_lists(c)[1]) for c in cases])
        assert out.getvalue() == g["text"], (i, g["keys"])
        assert len(g["text"].splitlines()) == 10


def test_summaries_equal_summary_row_by_row():
    """the one-pass form over a matrix writes what the value-by-value restatement of Stats.Summary writes"""
    from gat_amd import metrics
    r = np.random.RandomState(5)
    for k in (1, 2, 3, 4, 5, 7, 8, 24, 129, 300):
        ints = r.randint(0, 2 ** 40, size=(40, k)).astype(np.int64)
        ints[::3] //= 2 ** 30
        floats = r.random_sample((40, k)) * r.choice([1.0, 1e-3, 50.0], size=(40, 1))
        floats[::4, : k // 2] = 0.0
        for m in (ints, floats):
            got = metrics.summaries(m)
            assert got == [metrics.summary(row.tolist()) for row in m]
    assert metrics.summaries(np.zeros((3, 0), dtype=np.int64)) == [metrics.summary([])] * 3
    assert metrics.summary([]) == "0" + "\t0.0000" * 8
    assert metrics.HEADER == "track\tsection\tmetric\tnval\tmin\tmax\tmean\tmedian\tstddev\tsum\tq1\tq3\n"


def test_attributes_follow_from_the_words():
    from gat_amd import metrics
    for segs, ws in fuzz_cases(200, seed=4):
        w = M.words(segs, ws)
        want = M.attributes_from_words(w, M.total(ws))
        got = metrics.attributes(np.array(w, dtype=np.int64), M.total(ws))
        for name, v in zip(metrics.ATTRIBUTES, got):
            assert v.item() == want[name], (name, v, want[name])
    assert metrics.WORDS == M.WORDS
