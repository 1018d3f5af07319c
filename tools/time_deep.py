#!/usr/bin/env python
"""Time a deep run -- gat_amd.run(null_round_size=R): the samples drawn in rounds of R, each folded into eight integer words a
row by gat_null_fold (DESIGN.md section 5 "k_null_fold") -- beside the plain run it must not be slower than per sample.

Shape 1: the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one annotation track) with the annotator,
for R in --rounds and num_samples = 10 R.  Per R, alternating, --reps times each:
  * the plain run of R samples (run(num_samples=R): the count matrix held, the parent's path), end to end;
  * the deep run of 10 R samples end to end, and inside it per round b > 0 (round 0 is enqueued early and overlaps host work)
    the round's sampling -- host clock from Problem.enqueue to the return of Problem.wait -- and its fold -- device time between
    two HIP events recorded on the library's stream around gat_null_fold, and the host clock around the synchronous call.
Shape 2: --tracks annotation tracks (config 4's count: 1 000 rows) over config 4's segments at --wide-round samples a round,
three rounds: there the fold reads rows x R x 8 bytes, set against the rate at which the chip streams HBM (6.3 TB/s measured
for a copy, MI355X).  The words of the deep runs are checked: n = num_samples for every row, and the p-values of a deep run of
R samples in rounds of R / 4 equal the plain run's.

    python tools/time_deep.py [--rounds 10000,100000,1000000] [--reps 3] [--tracks 1000] [--wide-round 100000] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gat_amd                                   # noqa: E402
from gat_amd import _lib, synthetic              # noqa: E402

HBM_STREAM_TBS = 6.3                             # a float4 copy on the MI355X, measured


def _mmm(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def _hip():
    """the HIP runtime the library itself runs on (the one mapped into this process), for the events around the fold"""
    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = sorted(set(line.split()[-1] for line in f if "libamdhip64" in line))
    if not paths:
        raise RuntimeError("no HIP runtime is loaded in this process")
    H = C.CDLL(paths[0])
    H.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    H.hipEventSynchronize.argtypes = [C.c_void_p]
    H.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    H.hipEventDestroy.argtypes = [C.c_void_p]
    return H


def _hipchk(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: hipError %d" % (what, rc))


class _Probe(object):
    """host clocks around a deep run's rounds (enqueue .. wait) and HIP events around its folds"""

    def __init__(self, ctx):
        self.hip = _hip()
        self.stream = C.c_void_p(ctx.stream_handle())
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            _hipchk(self.hip.hipEventCreate(C.byref(e)), "hipEventCreate")
        self.sample_s, self.fold_dev_s, self.fold_host_s, self.t_enqueue = [], [], [], None
        self.saved = (_lib.Problem.enqueue, _lib.Problem.wait, _lib.Context.null_fold)

    def __enter__(self):
        enqueue, wait, fold = self.saved
        probe = self

        def p_enqueue(self, counters, seed, b, e, dev):
            probe.t_enqueue = time.perf_counter() if b > 0 else None
            return enqueue(self, counters, seed, b, e, dev)

        def p_wait(self):
            r = wait(self)
            if probe.t_enqueue is not None:
                probe.sample_s.append(time.perf_counter() - probe.t_enqueue)
                probe.t_enqueue = None
            return r

        def p_fold(self, *args):
            H, (ev0, ev1) = probe.hip, probe.ev
            t0 = time.perf_counter()
            _hipchk(H.hipEventRecord(ev0, probe.stream), "hipEventRecord")
            r = fold(self, *args)
            _hipchk(H.hipEventRecord(ev1, probe.stream), "hipEventRecord")
            _hipchk(H.hipEventSynchronize(ev1), "hipEventSynchronize")
            probe.fold_host_s.append(time.perf_counter() - t0)
            ms = C.c_float()
            _hipchk(H.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
            probe.fold_dev_s.append(ms.value * 1e-3)
            return r
        _lib.Problem.enqueue, _lib.Problem.wait, _lib.Context.null_fold = p_enqueue, p_wait, p_fold
        return self

    def __exit__(self, *exc):
        _lib.Problem.enqueue, _lib.Problem.wait, _lib.Context.null_fold = self.saved
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def _run(colls, num_samples, null_round_size=0, seed=7):
    segments, annotations, workspace = colls
    t0 = time.perf_counter()
    rows = gat_amd.run(segments, annotations, workspace, gat_amd.SamplerAnnotator(bucket_size=1, nbuckets=100000),
                       [gat_amd.CounterNucleotideOverlap()], gat_amd.UnconditionalWorkspace(), num_samples=num_samples,
                       random_seed=seed, null_round_size=null_round_size)
    return time.perf_counter() - t0, rows


def shape(ctx, colls, R, S, reps, n_rows, what):
    ms = lambda t: tuple(1e3 * x for x in t)  # noqa: E731
    # the same samples: a deep run of R samples in four rounds against the plain run
    _, plain = _run(colls, R)                                             # (also the warm-up of both paths)
    _, deep = _run(colls, R, max(1, R // 4))
    assert [(r.expected, r.pvalue, r.fold) for r in plain] == [(r.expected, r.pvalue, r.fold) for r in deep], "deep and plain rows differ"
    t_plain, t_deep, samp, fold_dev, fold_host = [], [], [], [], []
    for _ in range(reps):                                                 # alternating: both see the same neighbours on the host
        t_plain.append(_run(colls, R)[0])
        with _Probe(ctx) as p:
            t, rows = _run(colls, S, R)
        assert len(rows) == n_rows and all(r.nsamples == S and r.null_words[0] == S for r in rows)
        t_deep.append(t)
        samp += p.sample_s
        fold_dev += p.fold_dev_s[1:]                                      # (the folds of the rounds whose sampling was timed)
        fold_host += p.fold_host_s[1:]
    plain_m, deep_m, samp_m, fd_m, fh_m = _mmm(t_plain), _mmm(t_deep), _mmm(samp), _mmm(fold_dev), _mmm(fold_host)
    gb = n_rows * R * 8 / 1e9
    per_plain, per_deep = [1e6 * t / R for t in plain_m], [1e6 * t / S for t in deep_m]
    return [
        "%s: %d row(s), rounds of %d samples, %d samples in all; medians of %d runs / %d rounds (lowest .. highest):" % (what, n_rows, R, S, reps, len(samp)),
        "    a round's sampling (enqueue .. wait, host clock)   %10.2f ms  (%.2f .. %.2f)" % ms(samp_m),
        "    its fold, k_null_fold (HIP events on the stream)   %10.3f ms  (%.3f .. %.3f)   = %.2f %% of the round's sampling; %.3f GB read: %.2f TB/s (%.0f %% of the %.1f TB/s a copy streams)"
        % (ms(fd_m) + (100.0 * fd_m[0] / samp_m[0], gb, gb / 1e3 / fd_m[0], 100.0 * gb / 1e3 / fd_m[0] / HBM_STREAM_TBS, HBM_STREAM_TBS)),
        "        gat_null_fold, host clock around the call      %10.3f ms  (%.3f .. %.3f)" % ms(fh_m),
        "    deep run of %d samples end to end               %10.2f ms  (%.2f .. %.2f)   %.4f us a sample (%.4f .. %.4f)" % ((S,) + ms(deep_m) + tuple(per_deep)),
        "    plain run of %d samples end to end (the parent's path) %8.2f ms  (%.2f .. %.2f)   %.4f us a sample (%.4f .. %.4f)" % ((R,) + ms(plain_m) + tuple(per_plain)),
        "    deep / plain, time per sample: %.3f  (the plain run's own spread, highest / lowest: %.3f; the deep run's: %.3f)"
        % (per_deep[0] / per_plain[0], plain_m[2] / plain_m[1], deep_m[2] / deep_m[1]),
        "    outside the rounds' sampling (run - rounds x a round's sampling): plain %.2f ms per run of %d samples, deep %.2f ms per run of %d"
        % (1e3 * (plain_m[0] - samp_m[0]), R, 1e3 * (deep_m[0] - (S // R) * samp_m[0]), S),
        "        -- where the two differ per sample: the sampling is the same calls at the same rate on both paths (%.4f us a sample in a"
        % (1e6 * samp_m[0] / R),
        "        round); the plain run pays its observed counts, problem creation, the read-back of its matrix, gat_null_stats and result rows",
        "        once per %d samples, the deep run once per %d, with a fold and no read-back in place of the matrix's" % (R, S),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", default="10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--wide-round", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_deep.txt"))
    a = ap.parse_args()
    ctx = gat_amd.get_context()
    lines = ["a null deeper than a count matrix (gat-run.py --null-round-size, gat_null_fold), MI355X, one GPU",
             "    python tools/time_deep.py --rounds %s --reps %d --tracks %d --wide-round %d" % (a.rounds, a.reps, a.tracks, a.wide_round)]
    colls = synthetic.as_collections(synthetic.config("config2"))[:3]
    for R in [int(x) for x in a.rounds.split(",")]:
        lines += shape(ctx, colls, R, 10 * R, a.reps, 1, "config-2 geometry, annotator")
    if a.tracks > 0:
        cfg = synthetic.config("config4")
        cfg["annotations"] = cfg["annotations"][:a.tracks]
        colls = synthetic.as_collections(cfg)[:3]
        lines += shape(ctx, colls, a.wide_round, 3 * a.wide_round, max(1, a.reps - 1), len(cfg["annotations"]),
                       "config-4 geometry (100 000 segments), annotator")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
