"""Call lanes (GAT_CALL_LANES; include/gat_mi355.h): an asynchronous call enqueued while another problem's call is in flight runs
on a stream of the library's own, beside it.  The counts do not depend on it -- equal under 1 and 2 lanes and equal to the
oracle --, the caller's stream stays ordered against the call both ways, and nothing a call on one lane reads is freed or
rewritten by the host on behalf of another."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gat_amd import _lib
from oracle import oracle as O
import call_lanes_cases as cases
from test_hip_parity import _big_problem, _random_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = cases.ALL


# ---- the rule alone (no device) ----------------------------------------------------------------------------------
def test_lane_selection_rules():
    f = _lib.call_lane_for
    # nothing else in flight: the context's stream, whatever the lanes
    assert f(2, True, False, False, 0, [0, 0]) == -1
    # another problem's call in flight: the first idle lane
    assert f(2, True, False, False, 1, [0, 0]) == 0
    assert f(2, True, False, False, 1, [1, 0]) == 1
    assert f(2, True, False, False, 1, [0, 1]) == 0
    assert f(4, True, False, False, 3, [1, 1, 1, 0]) == 3
    # every lane busy: queued on the first
    assert f(2, True, False, False, 2, [1, 1]) == 0
    # no lanes: GAT_CALL_LANES below 2
    for n in (1, 0, -3):
        assert f(n, True, False, False, 1, [0, 0]) == -1
    # beyond four: four
    assert f(9, True, False, False, 5, [1, 1, 1, 1, 0, 0]) == 0
    assert f(9, True, False, False, 3, [1, 1, 1, 0]) == 3
    # the synchronous entry points, per-kernel timing, the caller's serial state: the context's stream
    assert f(2, False, False, False, 1, [0, 0]) == -1
    assert f(2, True, True, False, 1, [0, 0]) == -1
    assert f(2, True, False, True, 1, [0, 0]) == -1


# ---- on the device -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _view(host, counters):
    return [host[k].view(np.float64) if c == "nucleotide-density" else host[k] for k, c in enumerate(counters)]


def _read(ctx, P, counters, n, dev):
    host = np.empty((len(counters), P.n_tracks, n), dtype=np.int64)
    ctx.d2h(host, dev)
    return _view(host, counters)


def _same(got, want, what):
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def schedule_oracle():
    F = cases.flats()
    return [O.run_samples(F[f], counters, 900 + (i & 1), 1, i * cases.S, (i + 1) * cases.S)[0]
            for i, (_, f, counters) in enumerate(cases.SCHEDULE)]


@pytest.mark.gpu
def test_counts_equal_under_one_and_two_lanes_and_the_oracle(tmp_path, schedule_oracle):
    got = {}
    for lanes in ("1", "2"):
        out = str(tmp_path / ("lanes%s.npz" % lanes))
        env = dict(os.environ, GAT_CALL_LANES=lanes)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "call_lanes_cases.py"), out], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(out)
        got[lanes] = {k: z[k] for k in z.files}
    assert sorted(got["1"]) == sorted(got["2"]) == sorted("call%d" % i for i in range(len(cases.SCHEDULE)))
    for i, (_, _, counters) in enumerate(cases.SCHEDULE):
        a, b = got["1"]["call%d" % i], got["2"]["call%d" % i]
        assert np.array_equal(a, b), i
        _same(_view(b, counters), schedule_oracle[i], i)


@pytest.mark.gpu
def test_waits_out_of_order_and_the_same_problem_twice(ctx):
    rs = np.random.RandomState(21)
    fa, fb = _random_problem(rs, 3, 200, 3, True), _random_problem(rs, 4, 150, 2, False)
    S = 128
    wa = [O.run_samples(fa, ALL, 5, 1, lo, lo + S)[0] for lo in (0, S)]
    wb = O.run_samples(fb, ALL, 6, 1, 0, S)[0]
    A, B = _lib.Problem(ctx, fa), _lib.Problem(ctx, fb)
    da = [ctx.alloc(len(ALL) * A.n_tracks * S * 8) for _ in range(2)]
    db = ctx.alloc(len(ALL) * B.n_tracks * S * 8)
    A.enqueue(ALL, 5, 0, S, da[0])
    B.enqueue(ALL, 6, 0, S, db)
    B.wait()
    A.wait()
    _same(_read(ctx, B, ALL, S, db), wb, "B")
    _same(_read(ctx, A, ALL, S, da[0]), wa[0], "A")
    # A, then A' on the same problem: one call per problem -- refused while A is in flight, serial behind it after the wait
    B.enqueue(ALL, 6, 0, S, db)
    A.enqueue(ALL, 5, 0, S, da[0])
    with pytest.raises(ValueError):
        A.enqueue(ALL, 5, S, 2 * S, da[1])
    A.wait()
    A.enqueue(ALL, 5, S, 2 * S, da[1])          # (B still in flight: a lane again, not the one A just left necessarily)
    A.wait()
    B.wait()
    _same(_read(ctx, A, ALL, S, da[0]), wa[0], "A again")
    _same(_read(ctx, A, ALL, S, da[1]), wa[1], "A'")
    _same(_read(ctx, B, ALL, S, db), wb, "B again")
    one_at_a_time = A.sample_and_count(ALL, 5, S, 2 * S)
    _same(one_at_a_time, wa[1], "blocking")
    for d in da + [db]:
        ctx.free(d)
    A.close()
    B.close()


def _hip_runtime():
    """the HIP runtime the library has loaded, for the caller's own stream work (a second copy of it would not see the device)"""
    import ctypes
    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = sorted(set(line.split()[-1] for line in f if "libamdhip64" in line))
    assert paths, "the library is loaded, its runtime is not mapped?"
    return ctypes.CDLL(paths[0])


@pytest.mark.gpu
def test_fork_and_join_against_the_callers_stream():
    """the caller fills the count matrix on its stream in front of the call and copies it on its stream behind it, with two
    calls in flight: the copy holds the call's counts, the fill did not run over them"""
    import ctypes
    hip = _hip_runtime()
    vp = ctypes.c_void_p

    def chk(e):
        assert e == 0, "HIP error %d" % e

    stream = vp()
    chk(hip.hipStreamCreateWithFlags(ctypes.byref(stream), ctypes.c_uint(1)))           # hipStreamNonBlocking
    c = _lib.Context(0, stream=stream.value)
    rs = np.random.RandomState(33)
    flat = _random_problem(rs, 3, 250, 3, False)
    counters = ["nucleotide-overlap", "segment-overlap"]
    S, steps = 128, 4
    nbytes = len(counters) * flat["n_tracks"] * S * 8
    wants = [O.run_samples(flat, counters, 8, 1, i * S, (i + 1) * S)[0] for i in range(steps)]
    anno = _lib.Annotations(c, flat)
    Ps = [_lib.Problem(c, flat, annotations=anno) for _ in range(2)]
    bufs = [c.alloc(nbytes) for _ in range(2)]
    copies = [c.alloc(nbytes) for _ in range(steps)]
    junk_bytes = 256 << 20
    junk = c.alloc(junk_bytes)
    for i in range(steps):
        b = i & 1
        # (work in front of the fill: the fill has not run when the call is enqueued)
        chk(hip.hipMemsetAsync(vp(junk), ctypes.c_int(i), ctypes.c_size_t(junk_bytes), stream))
        chk(hip.hipMemsetAsync(vp(bufs[b]), ctypes.c_int(0x5A), ctypes.c_size_t(nbytes), stream))
        Ps[b].enqueue(counters, 8, i * S, (i + 1) * S, bufs[b])
        chk(hip.hipMemcpyAsync(vp(copies[i]), vp(bufs[b]), ctypes.c_size_t(nbytes), ctypes.c_int(3), stream))   # device to device
        if i > 0:
            Ps[1 - b].wait()
    Ps[(steps - 1) & 1].wait()
    chk(hip.hipStreamSynchronize(stream))
    for i in range(steps):
        _same(_read(c, Ps[0], counters, S, copies[i]), wants[i], i)
    for d in bufs + copies + [junk]:
        c.free(d)
    for P in Ps:
        P.close()
    anno.close()
    c.close()
    chk(hip.hipStreamDestroy(stream))


@pytest.mark.gpu
def test_overflow_and_several_batches_on_both_lanes(ctx, monkeypatch):
    """tiny slab regions and a scratch budget of a few samples: both problems' calls are several batches, some overflow and are
    laid out again inside gat_wait while the other problem's call runs on the other lane"""
    rs = np.random.RandomState(78)
    f1, f2 = _big_problem(rs, 500, 5), _random_problem(rs, 3, 300, 5, True)
    counters = ["nucleotide-overlap", "segment-overlap"]
    S, steps = 96, 4
    wants = [O.run_samples(f1 if (i & 1) == 0 else f2, counters, 32, 1, i * S, (i + 1) * S)[0] for i in range(steps)]
    P2 = _lib.Problem(ctx, f2)                                  # (laid out with room)
    monkeypatch.setitem(ctx.options, "GAT_TEST_SMALL_CAPS", "1")
    P1 = _lib.Problem(ctx, f1)                                  # (laid out tight: its batches overflow)
    monkeypatch.setitem(ctx.options, "GAT_SLAB_BYTES", "300000")
    Ps = [P1, P2]
    devs = [ctx.alloc(len(counters) * P.n_tracks * S * 8) for P in Ps]
    retried = batches = 0
    for i in range(steps):
        Ps[i & 1].enqueue(counters, 32, i * S, (i + 1) * S, devs[i & 1])
        if i > 0:
            st = Ps[(i - 1) & 1].wait()
            retried += st["n_retried"]
            batches = max(batches, st["n_batches"])
            _same(_read(ctx, Ps[(i - 1) & 1], counters, S, devs[(i - 1) & 1]), wants[i - 1], i - 1)
    st = Ps[(steps - 1) & 1].wait()
    _same(_read(ctx, Ps[(steps - 1) & 1], counters, S, devs[(steps - 1) & 1]), wants[steps - 1], steps - 1)
    assert retried > 0 and batches > 2 and st["n_batches"] > 2, (retried, batches, st)
    for d in devs:
        ctx.free(d)
    for P in Ps:
        P.close()


@pytest.mark.gpu
def test_scratch_grows_and_a_problem_closes_beside_a_call_in_flight(ctx):
    """while A's call is in flight: B's call needs more scratch than its last one had (the old blocks go back to the pool),
    B is closed with that call in flight (the close waits for it), and a new problem takes the blocks B left.  A's counts,
    and the new problem's, are the oracle's"""
    rs = np.random.RandomState(55)
    fa, fb = _big_problem(rs, 600, 4), _random_problem(rs, 3, 300, 3, True)
    SA, SB = 256, 192
    wa = O.run_samples(fa, ALL, 3, 1, 0, SA)[0]
    wb = O.run_samples(fb, ALL, 4, 1, 0, SB)[0]
    A, B = _lib.Problem(ctx, fa), _lib.Problem(ctx, fb)
    da, db = ctx.alloc(len(ALL) * A.n_tracks * SA * 8), ctx.alloc(len(ALL) * B.n_tracks * SB * 8)
    B.sample_and_count(["nucleotide-overlap"], 4, 0, 8)      # (B's scratch: eight samples)
    A.enqueue(ALL, 3, 0, SA, da)
    B.enqueue(ALL, 4, 0, SB, db)                             # (grown beside A's call)
    B.wait()
    _same(_read(ctx, B, ALL, SB, db), wb, "B")
    A.wait()
    _same(_read(ctx, A, ALL, SA, da), wa, "A")
    A.enqueue(ALL, 3, 0, SA, da)
    B.enqueue(ALL, 4, 0, SB, db)
    B.close()                                                # (with its call in flight, and A's)
    C = _lib.Problem(ctx, fb)
    dc = ctx.alloc(len(ALL) * C.n_tracks * SB * 8)
    C.enqueue(ALL, 4, 0, SB, dc)
    A.wait()
    C.wait()
    _same(_read(ctx, A, ALL, SA, da), wa, "A beside the close")
    _same(_read(ctx, C, ALL, SB, dc), wb, "C")
    for d in (da, db, dc):
        ctx.free(d)
    A.close()
    C.close()
