"""Which check refuses a call of the list reductions when one or two of its arguments are wrong
(tests/test_list_call_refusals_gpu.py).  TEST INFRASTRUCTURE ONLY.

The ten entry points -- the list call and the sample call of gat-distance, gat-local, gat-pairs, gat-geneset and gat-profile --
over one tiny problem: one list, two tracks, two groups (the problem's two contigs), ranges of two samples.  A case is an entry
point, the arguments it changes, and where it runs: on the problem whose sampled lists are not normalized, or while a call is
in flight on the problem.  Every case is refused, but for the few marked ok: those have nothing to write and say so.

SOME CASES ARE SAFE ONLY BECAUSE THE CALL IS REFUSED before it reads its lists or draws a sample: list-longer-than-a-word gives
offsets up to 2^32 - 2 over an array of three segments; the sumsq-overflow cases ask for 2^62 samples (gat-pairs, gat-geneset:
their bound on a value is small) or for four (gat-local: bin_size is at most 2^31, and 2^62 * S reaches 2^64 only at S = 4, so
this one range is longer than the two samples every other case keeps to); n-lists-times-groups and n-tracks-times-groups give
counts the arrays do not have.  A library that let one of them through would read beyond an array on the host, or sample all but
for ever on the GPU, rather than fail an assert: when a change makes one of these cases fail, look at the return code in the
failure before running the module again.

What a case returns and the whole text of gat_last_error are in tests/golden/list_call_refusals.json.  That file is RECORDED,
from a build of the commit BEFORE a change to these entry points, never from the code under test:

    GAT_LIB_PATH=<the earlier commit's libgat_mi355.so> python tests/list_call_refusal_cases.py --record

(needs the GPU: the calls take a context).  A case that is added later is recorded the same way.
"""
import collections
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sampler_edges as E  # noqa: E402
from gat_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "list_call_refusals.json")
SEED = 11
SENTINEL = -7777
ANNOTATOR, SEGMENTS = 0, 1

# the problem: two units, a contig each.  SamplerSegments leaves its lists neither sorted nor disjoint.
UNITS = [([(10, 20), (40, 55), (70, 90)], [(0, 200)]), ([(5, 9), (30, 36)], [(0, 100)])]


def problem(sampler):
    return E.units_flat(UNITS, sampler)


def seg(pairs):
    a = np.zeros(len(pairs), dtype=_lib.SEG)
    if len(pairs):
        a["start"], a["end"] = np.array(pairs, dtype=np.int64).T
    return a


def i64(*v):
    return np.array(v, dtype=np.int64)


def i32(*v):
    return np.array(v, dtype=np.int32)


# ---- the valid arguments: 1 list x 2 groups against 2 tracks x 2 groups -------------------------------------------------------------
BASE = dict(
    n=1, g=2, t=2, begin=0, end=2,
    lists=seg([(10, 20), (40, 55), (5, 9)]), lo=i64(0, 2, 3),
    annos=seg([(0, 15), (50, 60), (3, 7), (12, 18)]), ao=i64(0, 2, 3, 4, 4),
    direction=0, max_distance=1000,
    w=10, bo=i64(0, 20, 30),
    pieces=seg([(0, 30), (35, 60), (2, 8)]), po=i64(0, 2, 3), mo=i64(0, 1, 3, 4), members=i32(0, 0, 1, 2), n_genes=3,
    to=i64(0, 2, 3), term_genes=i32(0, 1, 2), n_terms=2,
    ps=np.array([15, 15, 50, 7], dtype=np.uint32), mi=np.array([0, 1, 0, 0], dtype=np.uint8), ko=i64(0, 3, 4, 4, 4), h=2, mode=0,
    obs=np.zeros(64, dtype=np.int64),
)
# the C signatures, by the names above (c: the context, prob: the problem, out: out_host; SEED and STATS are fixed)
SIGNATURES = {
    "gat_list_distances": "c lists lo n annos ao t g direction max_distance out",
    "gat_sample_distances": "c prob SEED begin end annos ao t direction max_distance out STATS",
    "gat_list_bin_overlaps": "c lists lo n annos ao t g w bo out",
    "gat_sample_bin_enrichment": "c prob SEED begin end annos ao t w bo obs out STATS",
    "gat_list_pair_hits": "c lists lo n annos ao t g out",
    "gat_sample_pair_enrichment": "c prob SEED begin end annos ao t obs out STATS",
    "gat_list_geneset_hits": "c lists lo n pieces po mo members n_genes to term_genes n_terms g out",
    "gat_sample_geneset_enrichment": "c prob SEED begin end pieces po mo members n_genes to term_genes n_terms obs out STATS",
    "gat_list_profile": "c lists lo n ps mi ko t g w h mode out",
    "gat_sample_profile_enrichment": "c prob SEED begin end ps mi ko t w h mode obs out STATS",
}

# ---- the defects -------------------------------------------------------------------------------------------------------------------
LO_DOWN, LO_NEG = dict(lo=i64(0, 3, 2)), dict(lo=i64(-1, 2, 3))
LISTS_UNNORMALIZED = dict(lists=seg([(10, 20), (15, 55), (5, 9)]))
AO_DOWN, AO_NEG = dict(ao=i64(0, 3, 2, 4, 4)), dict(ao=i64(-1, 2, 3, 4, 4))
TRACK_UNNORMALIZED = dict(annos=seg([(0, 15), (10, 60), (3, 7), (12, 18)]))
TRACKS_TOO_MANY = dict(t=2 ** 30)                     # x 2 groups: beyond 2^31 - 1
OBS_NEGATIVE = dict(obs=np.concatenate([i64(-3), np.zeros(63, dtype=np.int64)]))
BACKWARDS = dict(begin=3, end=2)
NO_TRACKS = dict(t=0, ao=i64(0))
Case = collections.namedtuple("Case", "id entry change ok problem in_flight")
CASES = []


def case(entry, name, *changes, **where):
    change = {}
    for c in changes:
        change.update(c)
    CASES.append(Case("%s-%s" % (entry.replace("gat_", ""), name), entry, change, where.get("ok", False),
                      where.get("problem", "annotator"), where.get("in_flight", False)))


def tool_cases(list_entry, sample_entry, singles, side_down, side_unnormalized, side_range, nothing, overflow, list_why_normalized,
               sample_needs_normalized, folds=True):
    """the cases of one tool.  singles: its own defects by name, for both calls; side_down / side_unnormalized / side_range: its
    offsets that decrease, its searched side that is not normalized, its count out of range; nothing: no track, no term;
    overflow: what makes sumsq overflow in the sample call"""
    L, S = list_entry, sample_entry
    for entry in (L, S):
        case(entry, "null-ctx", dict(c=None))
        case(entry, "null-out", dict(out=None))
        for name, change in singles.items():
            case(entry, name, change)
        case(entry, "nothing-no-side", nothing, ok=True)
        case(entry, "side-range+null-out", side_range, dict(out=None))
    # the list call: the NULLs, the counts, the tool's checks, the caller's lists
    case(L, "null-list-off", dict(lo=None))
    case(L, "null-lists", dict(lists=None))
    case(L, "n-lists-negative", dict(n=-1))
    case(L, "n-groups-negative", dict(g=-1))
    case(L, "n-lists-times-groups", dict(n=2 ** 30))
    case(L, "list-off-decreases", LO_DOWN)
    case(L, "list-off-negative", LO_NEG)
    if list_why_normalized is not None:
        case(L, "lists-unnormalized", LISTS_UNNORMALIZED, list_why_normalized)
        case(L, "side-down+lists-unnormalized", side_down, LISTS_UNNORMALIZED, list_why_normalized)
    case(L, "nothing-no-list", dict(n=0, lo=i64(0)), ok=True)
    case(L, "list-off-decreases+side-unnormalized", LO_DOWN, side_unnormalized)
    case(L, "n-lists-negative+side-range", dict(n=-1), side_range)
    case(L, "null-list-off+n-lists-negative", dict(lo=None, n=-1))
    case(L, "list-off-decreases+side-down", LO_DOWN, side_down)
    case(L, "in-flight+list-off-decreases", LO_DOWN, in_flight=True)
    # the sample call: the NULLs, the range, the tool's checks, obs, the sampler's lists, the call in flight
    case(S, "null-problem", dict(prob=None))
    case(S, "range-backwards", BACKWARDS)
    case(S, "range-backwards+side-down", BACKWARDS, side_down)
    case(S, "range-backwards+null-problem", BACKWARDS, dict(prob=None))
    case(S, "in-flight", in_flight=True)
    case(S, "in-flight+side-down", side_down, in_flight=True)
    case(S, "in-flight+range-backwards", BACKWARDS, in_flight=True)
    case(S, "unnormalized-problem+side-unnormalized", side_unnormalized, problem="segments")
    if sample_needs_normalized is not None:
        # (never with a call in flight: the only call that can be, the count, refuses such a problem itself)
        case(S, "unnormalized-problem", sample_needs_normalized, problem="segments")
    if folds:
        case(S, "null-obs", dict(obs=None))
        case(S, "obs-negative", OBS_NEGATIVE)
        case(S, "sumsq-overflow", overflow)
        case(S, "side-range+null-obs", side_range, dict(obs=None))
        case(S, "obs-negative+sumsq-overflow", OBS_NEGATIVE, overflow)
        case(S, "side-unnormalized+obs-negative", side_unnormalized, OBS_NEGATIVE)
        case(S, "unnormalized-problem+obs-negative", OBS_NEGATIVE, problem="segments")
        case(S, "unnormalized-problem+sumsq-overflow", overflow, problem="segments")
        case(S, "in-flight+obs-negative", OBS_NEGATIVE, in_flight=True)
    else:
        case(S, "nothing-empty-range", dict(begin=1, end=1), ok=True)
        case(S, "unnormalized-problem+side-down", sample_needs_normalized, side_down, problem="segments")


TRACK_SINGLES = collections.OrderedDict([
    ("null-anno-off", dict(ao=None)), ("null-annos", dict(annos=None)), ("n-tracks-negative", dict(t=-1)),
    ("n-tracks-times-groups", TRACKS_TOO_MANY), ("anno-off-decreases", AO_DOWN), ("anno-off-negative", AO_NEG),
    ("track-unnormalized", TRACK_UNNORMALIZED),
])


def with_singles(more):
    d = collections.OrderedDict(TRACK_SINGLES)
    d.update(more)
    return d


tool_cases("gat_list_distances", "gat_sample_distances",
           with_singles([("direction", dict(direction=2)), ("max-distance-negative", dict(max_distance=-1)),
                         ("max-distance-large", dict(max_distance=2 ** 32 + 1)), ("direction+n-tracks-negative", dict(direction=2, t=-1)),
                         ("max-distance-negative+anno-off-decreases", dict(max_distance=-1, ao=AO_DOWN["ao"])),
                         ("track-unnormalized-direction-1+anno-off-decreases", dict(direction=1, annos=TRACK_UNNORMALIZED["annos"], ao=AO_DOWN["ao"]))]),
           AO_DOWN, TRACK_UNNORMALIZED, dict(t=-1), NO_TRACKS, None, dict(direction=1), dict(direction=1), folds=False)
tool_cases("gat_list_bin_overlaps", "gat_sample_bin_enrichment",
           with_singles([("bin-size-zero", dict(w=0)), ("bin-size-large", dict(w=2 ** 31 + 1)), ("null-bin-off", dict(bo=None)),
                         ("bin-off-negative", dict(bo=i64(-1, 20, 30))), ("bin-off-decreases", dict(bo=i64(0, 20, 10))),
                         ("bin-size-zero+n-tracks-negative", dict(w=0, t=-1)),
                         ("bin-off-decreases+track-unnormalized", dict(bo=i64(0, 20, 10), annos=TRACK_UNNORMALIZED["annos"]))]),
           AO_DOWN, TRACK_UNNORMALIZED, dict(t=-1), NO_TRACKS, dict(w=2 ** 31, end=4), {}, {})
tool_cases("gat_list_pair_hits", "gat_sample_pair_enrichment",
           with_singles([("n-tracks-2049", dict(t=2049)), ("n-tracks-2049+anno-off-decreases", dict(t=2049, ao=AO_DOWN["ao"]))]),
           AO_DOWN, TRACK_UNNORMALIZED, dict(t=-1), NO_TRACKS, dict(end=2 ** 62), None, None)
case("gat_list_pair_hits", "n-tracks-times-groups-named", dict(t=2048, g=2 ** 21))
case("gat_list_pair_hits", "list-longer-than-a-word", dict(lo=i64(0, 2 ** 31 - 1, 2 ** 32 - 2)))
case("gat_list_pair_hits", "list-longer-than-a-word+track-unnormalized", dict(lo=i64(0, 2 ** 31 - 1, 2 ** 32 - 2)), TRACK_UNNORMALIZED)
GENES_UNNORMALIZED = dict(pieces=seg([(0, 30), (20, 60), (2, 8)]))
tool_cases("gat_list_geneset_hits", "gat_sample_geneset_enrichment",
           collections.OrderedDict([
               ("null-piece-off", dict(po=None)), ("null-member-off", dict(mo=None)), ("null-term-off", dict(to=None)),
               ("null-pieces", dict(pieces=None)), ("null-members", dict(members=None)), ("null-term-genes", dict(term_genes=None)),
               ("n-genes-negative", dict(n_genes=-1)), ("n-genes-large", dict(n_genes=262145)), ("n-terms-negative", dict(n_terms=-1)),
               ("piece-off-decreases", dict(po=i64(0, 3, 2))), ("pieces-unnormalized", GENES_UNNORMALIZED),
               ("member-off-negative", dict(mo=i64(-1, 1, 3, 4))), ("member-off-decreases", dict(mo=i64(0, 3, 1, 4))),
               ("piece-without-member", dict(mo=i64(0, 1, 1, 2))), ("members-descend", dict(members=i32(0, 1, 0, 2))),
               ("member-out-of-range", dict(members=i32(0, 0, 3, 2))), ("term-off-negative", dict(to=i64(-1, 2, 3))),
               ("term-off-decreases", dict(to=i64(0, 3, 2))), ("term-genes-descend", dict(term_genes=i32(1, 0, 2))),
               ("n-terms-negative+piece-off-decreases", dict(n_terms=-1, po=i64(0, 3, 2))),
               ("members-descend+term-off-decreases", dict(members=i32(0, 1, 0, 2), to=i64(0, 3, 2))),
               ("pieces-unnormalized+member-off-decreases", dict(pieces=GENES_UNNORMALIZED["pieces"], mo=i64(0, 3, 1, 4))),
           ]),
           dict(po=i64(0, 3, 2)), GENES_UNNORMALIZED, dict(n_genes=-1), dict(n_terms=0, to=i64(0)), dict(end=2 ** 62), None, None)
ANCHORS_OUT_OF_ORDER = dict(ps=np.array([15, 15, 14, 7], dtype=np.uint32))
tool_cases("gat_list_profile", "gat_sample_profile_enrichment",
           collections.OrderedDict([
               ("null-anchor-off", dict(ko=None)), ("null-anchor-pos", dict(ps=None)), ("null-anchor-minus", dict(mi=None)),
               ("bin-size-zero", dict(w=0)), ("bin-size-large", dict(w=2 ** 31 + 1)), ("half-bins-zero", dict(h=0)),
               ("half-bins-513", dict(h=513)), ("reach-large", dict(h=512, w=2 ** 22 + 1)), ("mode", dict(mode=2)),
               ("n-tracks-negative", dict(t=-1)), ("n-tracks-times-groups", TRACKS_TOO_MANY),
               ("anchor-off-decreases", dict(ko=i64(0, 4, 3, 4, 4))), ("anchor-off-negative", dict(ko=i64(-1, 3, 4, 4, 4))),
               ("anchor-minus-2", dict(mi=np.array([0, 2, 0, 0], dtype=np.uint8))),
               ("anchor-repeats", dict(mi=np.array([0, 0, 0, 0], dtype=np.uint8))), ("anchors-out-of-order", ANCHORS_OUT_OF_ORDER),
               ("value-beyond-32-bits", dict(w=2 ** 31, h=1)),
               ("mode+anchor-off-decreases", dict(mode=2, ko=i64(0, 4, 3, 4, 4))),
               ("anchors-out-of-order+value-beyond-32-bits", dict(ps=ANCHORS_OUT_OF_ORDER["ps"], w=2 ** 31, h=1)),
           ]),
           dict(ko=i64(0, 4, 3, 4, 4)), ANCHORS_OUT_OF_ORDER, dict(t=-1), dict(t=0, ko=i64(0)),
           dict(w=(2 ** 32 - 1) // 4, h=1), {}, {})
case("gat_list_profile", "value-beyond-32-bits+lists-unnormalized", dict(w=2 ** 31, h=1), LISTS_UNNORMALIZED)
assert len({c.id for c in CASES}) == len(CASES)


# ---- running a case ----------------------------------------------------------------------------------------------------------------
class Env(object):
    """a context, the two problems, and the sentinel-filled out_host of every call"""

    def __init__(self):
        self.L = _lib.lib()
        self.ctx = _lib.Context(0)
        self.problems = {"annotator": _lib.Problem(self.ctx, problem(ANNOTATOR)), "segments": _lib.Problem(self.ctx, problem(SEGMENTS))}
        self.out = np.full(4096, SENTINEL, dtype=np.int64)

    def close(self):
        for P in self.problems.values():
            P.close()
        self.ctx.close()

    def call(self, entry, change, problem_name="annotator"):
        args = dict(BASE, c=self.ctx._h, prob=self.problems[problem_name]._h, out=self.out)
        args.update(change)
        values = []
        for name in SIGNATURES[entry].split():
            v = SEED if name == "SEED" else None if name == "STATS" else args[name]
            values.append(_lib._p(v) if isinstance(v, np.ndarray) else v)
        return getattr(self.L, entry)(*values)

    def run(self, c):
        """(return code, gat_last_error -- the thread's where the case has no context --, out_host as the call left it)"""
        self.out[:] = SENTINEL
        P = self.problems[c.problem]
        if c.in_flight:
            dev = self.ctx.alloc(8)
            P.enqueue(["nucleotide-overlap"], SEED, 0, 2, dev)
        try:
            rc = self.call(c.entry, c.change, c.problem)
            text = self.L.gat_last_error(None if "c" in c.change else self.ctx._h).decode()
        finally:
            if c.in_flight:
                P.wait()
                self.ctx.free(dev)
        return rc, text, self.out.copy()


def record(path):
    """the cases against the library GAT_LIB_PATH names: the commit before the change under test"""
    if not os.environ.get("GAT_LIB_PATH"):
        raise SystemExit("record from the parent commit's library: set GAT_LIB_PATH to it (never the code under test)")
    env = Env()
    got = collections.OrderedDict()
    try:
        for c in CASES:
            rc, text, out = env.run(c)
            assert (rc == 0) == c.ok, (c.id, rc, text)
            assert (out == SENTINEL).all(), c.id
            got[c.id] = dict(rc=rc, error="" if c.ok else text)
            assert env.call(c.entry, {}) == 0, c.id
    finally:
        env.close()
    with open(path, "w") as f:
        json.dump(dict(library=_lib.lib().gat_version().decode(), cases=got), f, indent=1)
        f.write("\n")
    print("recorded %d cases from %s into %s" % (len(got), _lib.LIB_PATH, path))


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        raise SystemExit("usage: GAT_LIB_PATH=<parent commit's library> python tests/list_call_refusal_cases.py --record [FILE]")
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
