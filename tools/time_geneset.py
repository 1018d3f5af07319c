#!/usr/bin/env python
"""Time gat_sample_geneset_enrichment on the config-2 geometry (synthetic.config("config2"): hg19, 10 000 segments, one workspace
segment per contig), SamplerAnnotator, against --genes synthetic genes of mixed length that overlap each other, for every
--terms (a term holds --per-gene * genes / terms genes on average, sizes drawn log-uniformly around that):

  (a) the call end to end (wall clock around Problem.sample_geneset_enrichment: the pieces, members, terms and obs up, the
      sampler, k_geneset_hits and k_geneset_terms behind every batch, k_null_finish, the five words per term down),
  (b) gat_stats::ms_sampler of the same call -- the sampler's kernels alone,
  (c) the same call over ONE sample -- the fixed cost of a call, so (a) - (b) - (c) is close to what the two kernels cost over
      the samples,
  (e) gat_sample_distances, direction 0, on ONE track that holds the same pieces, with its own (b) and (c): one search per
      segment, the yardstick of the search phase,
  (d) the route there was before: Problem.sample (every list copied to the host) and numpy over the lists, on --host-samples
      samples, scaled.

Medians over the repeats; the first call warms up.  The words of (a)'s route and (d) over the host route's samples are compared
on the way.

    python tools/time_geneset.py [--samples 10000] [--host-samples 20] [--genes 20000] [--terms 1000 --terms 10000]
                                 [--per-gene 5 --per-gene 50] [--reps 3] [--out profiles/r20_geneset.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gat_amd import _lib, geneset, intervals, problem, synthetic     # noqa: E402


def draw_genes(n, contigs, seed):
    """n genes of one interval each, uniformly over the genome; lengths geometric around 2 kb, 30 kb and 300 kb in equal parts"""
    rs = np.random.RandomState(seed)
    names = list(contigs)
    sizes = np.array([synthetic.HG19[c] for c in names], dtype=np.int64)
    cum = np.cumsum(sizes)
    pos = rs.randint(0, cum[-1], size=n).astype(np.int64)
    length = rs.geometric(1.0 / np.array([2000.0, 30000.0, 300000.0])[rs.randint(0, 3, size=n)]).astype(np.int64)
    ci = np.searchsorted(cum, pos, side="right")
    start = pos - (cum[ci] - sizes[ci])
    end = np.minimum(start + length, sizes[ci])
    return [{names[ci[g]]: intervals.make([start[g]], [end[g]])} for g in range(n)]


def draw_terms(n_terms, n_genes, per_gene, seed):
    """sizes log-uniform between a tenth and ten times the mean (at least 1, at most all genes), genes without replacement"""
    rs = np.random.RandomState(seed)
    mean = per_gene * n_genes / float(n_terms)
    draw = np.exp(rs.uniform(np.log(mean / 10.0), np.log(mean * 10.0), size=n_terms)) / 2.15        # (2.15: the mean of exp(U) over the mean)
    sizes = np.clip(draw, 1, n_genes).astype(np.int64)
    lists = [np.sort(rs.choice(n_genes, size=int(k), replace=False)).astype(np.int32) for k in sizes]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.concatenate(lists).astype(np.int32)


def host_route(P, seed, n_samples, pieces, piece_off, member_off, members, n_genes, term_off, term_genes, obs):
    """Returns (int64 [T, 5], segments copied)"""
    seg, off = P.sample(seed, 0, n_samples)
    C, T = P.n_contigs, len(term_off) - 1
    out = np.zeros((T, 5), dtype=np.int64)
    sizes = np.diff(term_off)
    for i in range(n_samples):
        H = np.zeros(n_genes + 1, dtype=np.int64)
        for c in range(C):
            a = seg[off[i * C + c]:off[i * C + c + 1]]
            p = pieces[piece_off[c]:piece_off[c + 1]]
            if len(a) == 0 or len(p) == 0:
                continue
            j0 = np.searchsorted(p["end"], a["start"], side="right") + piece_off[c]
            j1 = np.maximum(np.searchsorted(p["start"], a["end"], side="left") + piece_off[c], j0)
            m0, m1 = member_off[j0], member_off[j1]
            cnt = m1 - m0
            idx = np.repeat(m0, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            H[members[idx]] = 1
        run = np.concatenate([[0], np.cumsum(H[term_genes])])
        v = np.where(sizes > 0, run[term_off[1:]] - run[term_off[:-1]], 0)
        out[:, 0] += v > 0
        out[:, 1] += v
        out[:, 2] += v * v
        out[:, 3] += v < obs
        out[:, 4] += v == obs
    return out, len(seg)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=20)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--terms", type=int, action="append")
    ap.add_argument("--per-gene", type=float, action="append", help="terms a gene sits in, on average; one value per --terms")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_geneset.txt"))
    a = ap.parse_args()
    n_terms = a.terms or [1000, 10000]
    per_gene = a.per_gene or [5.0, 50.0]
    assert len(per_gene) == len(n_terms)
    cfg = synthetic.config("config2")
    flat = problem.flatten_arrays(cfg["segments"], [], cfg["workspace"], None)
    contigs = list(flat["contig_names"])
    segs = [intervals.normalize(cfg["segments"][c]) if c in cfg["segments"] else intervals.EMPTY for c in contigs]
    seg_all = np.concatenate(segs)
    seg_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    G = a.genes
    t0 = time.perf_counter()
    pieces, piece_off, member_off, members = geneset.flatten_genes(draw_genes(G, contigs, 300), contigs)
    ms_flatten = (time.perf_counter() - t0) * 1e3
    per_piece = np.diff(member_off)
    ctx = _lib.Context(0)
    ctx.set_kernel_times(True)
    P = _lib.Problem(ctx, flat)
    lines = ["python tools/time_geneset.py --samples %d --host-samples %d --genes %d %s %s --reps %d" % (
                 a.samples, a.host_samples, G, " ".join("--terms %d" % t for t in n_terms), " ".join("--per-gene %g" % x for x in per_gene), a.reps),
             "gat_sample_geneset_enrichment on the config-2 geometry: %d units, %d segments, SamplerAnnotator, %d samples, MI355X, one GPU" % (
                 flat["n_units"], len(flat["segs"]), a.samples),
             "%d genes -> %d pieces, %d member entries, at most %d genes a piece (flatten_genes: %.0f ms on the host)" % (
                 G, len(pieces), len(members), int(per_piece.max()), ms_flatten)]
    # (e) the yardstick: one search per segment into one track that holds the pieces
    d_wall, d_sampler, d_fixed = [], [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        P.sample_distances(7, 0, a.samples, pieces, piece_off, 1, 0, 0)
        d_wall.append((time.perf_counter() - t0) * 1e3)
        d_sampler.append(P.last_stats["ms_sampler"])
        t0 = time.perf_counter()
        P.sample_distances(7, 0, 1, pieces, piece_off, 1, 0, 0)
        d_fixed.append((time.perf_counter() - t0) * 1e3)
    (ms_e, e0, e1), (ms_eb, _, _), (ms_ec, _, _) = median(d_wall[1:]), median(d_sampler[1:]), median(d_fixed[1:])
    k_distance = ms_e - ms_eb - ms_ec
    lines += ["    (e) gat_sample_distances, direction 0, one track of the pieces, end to end %9.1f ms  (%.1f .. %.1f); its sampler %.1f ms, "
              "over one sample %.1f ms" % (ms_e, e0, e1, ms_eb, ms_ec),
              "        k_distance over the samples (one search per segment) %8.1f ms" % k_distance]
    kernels = []
    for T, pg in zip(n_terms, per_gene):
        term_off, term_genes = geneset.with_all_genes(*draw_terms(T, G, pg, 500 + T), n_genes=G)
        T1 = T + 1
        t0 = time.perf_counter()
        obs = ctx.list_geneset_hits(seg_all, seg_off, 1, pieces, piece_off, member_off, members, G, term_off, term_genes, T1, len(contigs))[0]
        ms_obs = (time.perf_counter() - t0) * 1e3
        args = (pieces, piece_off, member_off, members, G, term_off, term_genes, T1, obs)
        wall, sampler, fixed = [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = P.sample_geneset_enrichment(7, 0, a.samples, *args)
            wall.append((time.perf_counter() - t0) * 1e3)
            sampler.append(P.last_stats["ms_sampler"])
            batches = P.last_stats["n_batches"]
            t0 = time.perf_counter()
            P.sample_geneset_enrichment(7, 0, 1, *args)
            fixed.append((time.perf_counter() - t0) * 1e3)
        (ms_a, a0, a1), (ms_b, b0, b1), (ms_c, c0, c1) = median(wall[1:]), median(sampler[1:]), median(fixed[1:])
        k_geneset = ms_a - ms_b - ms_c
        kernels.append(k_geneset)
        part = P.sample_geneset_enrichment(7, 0, a.host_samples, *args)
        t0 = time.perf_counter()
        host, n_seg = host_route(P, 7, a.host_samples, pieces, piece_off, member_off, members, G, term_off, term_genes, obs)
        ms_host = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(host, part)
        ms_d = ms_host * a.samples / a.host_samples
        sizes = np.diff(term_off)[:-1]
        lines += [
            "%d terms (and the pseudo-term of all genes): %d gene entries, %.1f terms a gene, median term %d genes, largest %d; the input "
            "segments hit %d genes (gat_list_geneset_hits: %.1f ms), a sample %.1f on average; %d batches" % (
                T, int(term_off[-2]), term_off[-2] / float(G), int(np.median(sizes)), int(sizes.max()), int(obs[-1]), ms_obs,
                got[-1, 1] / float(a.samples), batches),
            "    (a) gat_sample_geneset_enrichment end to end        %9.1f ms  (%.1f .. %.1f)" % (ms_a, a0, a1),
            "    (b) ms_sampler of the same call                     %9.1f ms  (%.1f .. %.1f)" % (ms_b, b0, b1),
            "    (c) the same call over one sample (genes, terms and obs up, words down) %9.1f ms  (%.1f .. %.1f)" % (ms_c, c0, c1),
            "        (a) - (b) - (c): the two kernels over the samples %7.1f ms = %.2f x the sampler = %.2f x k_distance" % (
                k_geneset, k_geneset / max(ms_b, 1e-9), k_geneset / max(k_distance, 1e-9)),
            "    (d) Problem.sample + numpy, %d samples: %.1f ms (%d segments), scaled to %d samples %9.1f ms" % (
                a.host_samples, ms_host, n_seg, a.samples, ms_d),
            "        (d) / (a) = %.1f; the two routes' words over those %d samples are %s" % (ms_d / ms_a, a.host_samples,
                                                                                            "equal" if same else "DIFFERENT"),
        ]
        assert same
    if len(kernels) >= 2:
        lines.append("the kernels' time grows %.2f x from %d to %d terms (%.1f x the gene entries)" % (
            kernels[-1] / max(kernels[0], 1e-9), n_terms[0], n_terms[-1], (per_gene[-1] / per_gene[0])))
    P.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
