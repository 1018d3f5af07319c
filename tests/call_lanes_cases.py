"""The scenario tests/test_call_lanes.py runs under GAT_CALL_LANES=1 and =2 in fresh processes: calls of four problems taking
turns in flight.  Run as a script it writes every call's count matrix to an .npz; imported, it hands out the same problems
and the same schedule so the parent can ask the oracle about them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ALL = ["nucleotide-overlap", "nucleotide-density", "segment-overlap", "annotation-overlap"]
NUC = ["nucleotide-overlap", "nucleotide-density"]
S = 128


def flats():
    """x: the inputs two problems share (one set of annotation tables); y: an isochore problem of five tracks (nucleotide
    counters: the merged index, the units' lists counted directly, else k_contig); z: plain contigs"""
    from test_hip_parity import _random_problem
    rs = np.random.RandomState(4242)
    return {"x": _random_problem(rs, 4, 300, 3, False), "y": _random_problem(rs, 3, 250, 5, True),
            "z": _random_problem(rs, 3, 120, 2, False)}


# (problem, inputs, counters) per call; call i draws samples [i * S, (i + 1) * S) with seed 900 + (i & 1)
SCHEDULE = [("x1", "x", ALL), ("x2", "x", ALL), ("x1", "x", ALL), ("x2", "x", ALL),
            ("y", "y", NUC), ("z", "z", ALL), ("y", "y", ALL), ("z", "z", ALL), ("x1", "x", NUC)]


def run(ctx):
    """every call enqueued before the one in front of it is waited for: two calls in flight throughout"""
    from gat_amd import _lib
    F = flats()
    anno = _lib.Annotations(ctx, F["x"])
    Ps = {"x1": _lib.Problem(ctx, F["x"], annotations=anno), "x2": _lib.Problem(ctx, F["x"], annotations=anno),
          "y": _lib.Problem(ctx, F["y"]), "z": _lib.Problem(ctx, F["z"])}
    out, devs = {}, []

    def finish(i):
        name, _, counters = SCHEDULE[i]
        P = Ps[name]
        P.wait()
        host = np.empty((len(counters), P.n_tracks, S), dtype=np.int64)
        ctx.d2h(host, devs[i])
        out["call%d" % i] = host

    for i, (name, _, counters) in enumerate(SCHEDULE):
        P = Ps[name]
        devs.append(ctx.alloc(len(counters) * P.n_tracks * S * 8))
        P.enqueue(counters, 900 + (i & 1), i * S, (i + 1) * S, devs[i])
        if i > 0:
            finish(i - 1)
    finish(len(SCHEDULE) - 1)
    for d in devs:
        ctx.free(d)
    for P in Ps.values():
        P.close()
    anno.close()
    return out


if __name__ == "__main__":
    from gat_amd import _lib
    c = _lib.Context(0)
    np.savez(sys.argv[1], **run(c))
    c.close()
