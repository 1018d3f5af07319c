"""CPU: gat-geneset's host side -- the gene file and the map as they are read, the terms' CSR, the hypergeometric columns, which rows
are written and how, q-values per track, what is refused, and the identity the GPU test against the count stage rests on."""
import importlib.util
import io
import os
import random

import numpy as np
import pytest

import geneset_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def script():
    spec = importlib.util.spec_from_file_location("gat_geneset_cli", os.path.join(ROOT, "scripts", "gat-geneset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_cli_genes(tmp_path):
    """a gene file and a map for the inputs of tests/golden/cli: three consecutive intervals of annotations.bed, each 300 bases
    longer, are one gene (so genes overlap, and some lie outside the workspace); seven terms, one of a single gene, and in the
    map a comment, a repeated line and an id the gene file lacks"""
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(CLI, "annotations.bed")) if not l.startswith("track")]
    genes_file, map_file = str(tmp_path / "genes.bed"), str(tmp_path / "gene2term.tsv")
    with open(genes_file, "w") as f:
        f.write("# contig start end gene\n")
        for i, (contig, start, end) in enumerate(r[:3] for r in rows):
            f.write("%s\t%s\t%d\tg%03d\t0\t+\n" % (contig, start, int(end) + 300, i // 3))
    n = (len(rows) + 2) // 3
    with open(map_file, "w") as f:
        f.write("gene_id\tterm\n# a comment\n")
        for k in range(n):
            f.write("g%03d\tT%d\n" % (k, k % 5))
            if k % 7 == 0:
                f.write("g%03d\tT5\n" % k)
        f.write("g%03d\tT6\ng000\tT0\nnope\tT0\n" % (n // 2))
    return genes_file, map_file


def test_gene_file_and_map_as_read(tmp_path):
    from gat_amd import geneset
    from gat_amd import io as IO
    bed = tmp_path / "genes.bed"
    bed.write_text("# a comment\nc1\t10\t30\tA\t0\t+\nc1\t20\t50\tA\nc2\t5\t9\tB\nc1\t40\t60\tC\nc1\t10\t30\tA\nc2\t7\t8\tD\n")
    coll = IO.readSegmentList("annotations", [str(bed)])
    coll.normalize()
    ids, genes, dropped = geneset.gene_table(coll)
    assert ids == ["A", "B", "C", "D"] and dropped == 0                      # lines with the same id are one gene
    assert [dict((c, [tuple(x) for x in a.tolist()]) for c, a in g.items()) for g in genes] == [
        {"c1": [(10, 50)]}, {"c2": [(5, 9)]}, {"c1": [(40, 60)]}, {"c2": [(7, 8)]}]
    pieces, piece_off, member_off, members = geneset.flatten_genes(genes, ["c1", "c2"])
    assert [tuple(x) for x in pieces.tolist()] == [(10, 40), (40, 50), (50, 60), (5, 7), (7, 8), (8, 9)]
    assert piece_off.tolist() == [0, 3, 6] and members.tolist() == [0, 0, 2, 2, 1, 1, 3, 1]
    # a gene left with no base is dropped and counted
    coll["C"]["c1"].intersect(coll["B"]["c2"])
    assert geneset.gene_table(coll)[0] == ["A", "B", "D"] and geneset.gene_table(coll)[2] == 1
    tsv = tmp_path / "map.tsv"
    tsv.write_text("# comment before the header\ngene\tterm\nA\tt1\nB\tt1\n# comment\nA\tt2\nA\tt1\n\nZ\tt2\nZ\tt3\nD\tt1\tignored\nQ\tt2\n")
    sets = geneset.read_gene_sets(str(tsv))
    assert list(sets.items()) == [("t1", ["A", "B", "D"]), ("t2", ["A", "Z", "Q"]), ("t3", ["Z"])]
    terms, term_off, term_genes, unknown = geneset.term_table(sets, ["A", "B", "D"])
    assert terms == ["t1", "t2", "t3"] and term_off.tolist() == [0, 3, 4, 4] and term_genes.tolist() == [0, 1, 2, 0] and unknown == 2
    assert term_off.dtype == np.int64 and term_genes.dtype == np.int32
    off, all_genes = geneset.with_all_genes(term_off, term_genes, 3)
    assert off.tolist() == [0, 3, 4, 4, 7] and all_genes.tolist() == [0, 1, 2, 0, 0, 1, 2] and all_genes.dtype == np.int32
    assert geneset.term_table(sets, [])[1:] [0].tolist() == [0, 0, 0, 0]
    (tmp_path / "short.tsv").write_text("gene\tterm\nA\n")
    with pytest.raises(IOError, match="malformatted"):
        geneset.read_gene_sets(str(tmp_path / "short.tsv"))


def test_hypergeometric_columns():
    from gat_amd import geneset
    # N = 10 genes, K = 4 carry the term, n = 3 are hit, k = 2 of those carry it: P(X >= 2) = (C(4,2) C(6,1) + C(4,3)) / C(10,3)
    expected, fold, pvalue = geneset.hypergeometric(2, 10, 4, 3)
    assert expected == 1.2 and fold == 2 / 1.2 and abs(pvalue - (6 * 6 + 4) / 120.0) < 1e-12
    assert abs(geneset.hypergeometric(0, 10, 4, 3)[2] - 1.0) < 1e-12 and geneset.hypergeometric(0, 10, 4, 3)[1] == 0.0
    assert abs(geneset.hypergeometric(3, 10, 4, 3)[2] - 4 / 120.0) < 1e-12
    for k, N, K, n in ((0, 10, 4, 0), (0, 0, 0, 0), (0, 10, 0, 3)):
        got = geneset.hypergeometric(k, N, K, n)
        assert got == (0, 1.0, 1.0) and isinstance(got[0], int)


def hand_table(min_term_genes=1):
    from gat_amd import geneset
    S = 4
    names = ["a", "b", "c", "d"]
    term_off = [0, 4, 5, 5, 8]                                  # K = 4, 1, 0, 3
    v = np.zeros((S, 5), dtype=np.int64)
    v[:, 0] = [0, 3, 3, 10]                                     # a
    v[:, 1] = [1, 0, 0, 0]                                      # b: sampled only
    v[:, 3] = [2, 3, 3, 2]                                      # d
    v[:, 4] = [4, 5, 5, 10]                                     # all genes
    obs = np.array([3, 0, 0, 1, 6], dtype=np.int64)
    return geneset.rows("trk", names, term_off, 12, obs, M.words(v, obs), S, min_term_genes=min_term_genes), geneset


def test_rows_selection_and_format():
    res, geneset = hand_table(min_term_genes=0)
    assert [(x.annotation, x.genes_in_workspace, x.genes_with_annotation, x.genes_with_segments, x.observed, x.samples_with_hit) for x in res] == [
        ("a", 12, 4, 6, 3, 3), ("b", 12, 1, 6, 0, 1), ("c", 12, 0, 6, 0, 0), ("d", 12, 3, 6, 1, 4)]
    a, b, c, d = res
    assert (a.expected, a.pvalue, a.fold, a.expected_genes_with_segments) == (4.0, 0.75, 4.0 / 5.0, 6.0)
    assert (b.expected, b.fold, b.pvalue) == (0.25, 1.0 / 1.25, 0.75)
    assert (c.expected, c.stddev, c.fold, c.pvalue) == (0.0, 0.0, 1.0, 1.0)
    assert (c.hypergeom_expected, c.hypergeom_fold, c.hypergeom_pvalue) == (0, 1.0, 1.0)
    assert a.hypergeom_expected == 2.0 and a.hypergeom_fold == 1.5 and (d.expected, d.pvalue) == (2.5, 0.25)
    geneset.set_qvalues(res, "none")
    want_p = (15 * 28 + 20 * 8 + 15 * 1) / 924.0                # P(X >= 3), N = 12, K = 4, n = 6: C(4,3) C(8,3) + C(4,4) C(8,2) over C(12,6)
    assert abs(a.hypergeom_pvalue - (4 * 56 + 28) / 924.0) < 1e-12 and want_p > 0
    assert str(a) == ("trk\ta\t12\t4\t6\t3\t4.0000\t0.8000\t7.5000e-01\t7.5000e-01\t3.6742\t-0.3219\t3\t6.0000\t2.0000\t1.5000\t%6.4e"
                      % a.hypergeom_pvalue)
    assert [x.annotation for x in hand_table(min_term_genes=2)[0]] == ["a", "d"]
    assert [x.annotation for x in hand_table()[0]] == ["a", "b", "d"]                   # the default: a term without a gene is not tested
    sink = io.StringIO()
    geneset.write_results(sink, res, "pvalue")
    lines = sink.getvalue().splitlines()
    assert lines[0].split("\t") == list(geneset.HEADER) and len(geneset.HEADER) == 17
    assert lines[0].split("\t")[:10] == ["track", "annotation", "genes_in_workspace", "genes_with_annotation", "genes_with_segments",
                                         "genes_with_annotation_and_segments", "expected", "fold", "pvalue", "qvalue"]
    assert [l.split("\t")[1] for l in lines[1:]] == ["d", "a", "b", "c"]                                     # (ties keep the terms' order)
    sink = io.StringIO()
    geneset.write_results(sink, list(reversed(res)), "track")
    assert [l.split("\t")[1] for l in sink.getvalue().splitlines()[1:]] == ["a", "b", "c", "d"]
    with pytest.raises(ValueError, match="unknown sort order"):
        geneset.write_results(io.StringIO(), res, "nothing")


def test_qvalues_per_track():
    from gat_amd import stats
    res, geneset = hand_table(min_term_genes=0)
    more, _ = hand_table(min_term_genes=0)
    for x in more[:2]:
        x.track = "other"
    family = res + more[:2]
    geneset.set_qvalues(family, "BH")
    assert [x.qvalue for x in res] == stats.adjustPValues([x.pvalue for x in res], method="BH").tolist()
    assert [x.qvalue for x in more[:2]] == stats.adjustPValues([x.pvalue for x in more[:2]], method="BH").tolist()
    geneset.set_qvalues(res, "bonferroni")
    assert [x.qvalue for x in res] == [1.0, 1.0, 1.0, 1.0]
    for bad in ("storey", "minp", "efdr"):
        with pytest.raises(ValueError, match="qvalue-method"):
            geneset.set_qvalues(family, bad)


def test_parser_and_what_is_refused(capsys):
    import gat_amd
    from gat_amd import geneset
    mod = script()
    opts, args = mod.buildParser().parse_args([])
    assert args == [] and opts.sampler == "annotator" and opts.qvalue_method == "BH" and opts.min_term_genes == 1 and opts.gene_sets is None
    assert opts.num_samples == 1000 and opts.pseudo_count == 1.0
    opts, _ = mod.buildParser().parse_args(["--segments=s.bed", "--genes=g.bed", "--workspace=w.bed", "--isochores=i.bed", "-m", "map.tsv",
                                            "--sampler=shift", "--num-samples=20", "--random-seed=4", "--order=fold", "--min-term-genes=5",
                                            "-q", "holm", "--pseudo-count=0.5", "--device=1", "--with-segment-tracks"])
    assert (opts.segment_files, opts.annotation_files, opts.workspace_files, opts.isochore_files) == (["s.bed"], ["g.bed"], ["w.bed"], ["i.bed"])
    assert (opts.sampler, opts.num_samples, opts.random_seed, opts.output_order, opts.qvalue_method, opts.pseudo_count, opts.device,
            opts.min_term_genes, opts.gene_sets, opts.ignore_segment_tracks) == ("shift", 20, 4, "fold", "holm", 0.5, 1, 5, "map.tsv", False)
    assert mod.buildParser().parse_args(["--annotations=a.bed", "--gene-sets=x"])[0].annotation_files == ["a.bed"]
    for name in gat_amd.CLI_SAMPLERS:
        assert mod.buildParser().parse_args(["--sampler=%s" % name])[0].sampler == name
    for name in geneset.QVALUE_METHODS:
        assert mod.buildParser().parse_args(["--qvalue-method=%s" % name])[0].qvalue_method == name
    for bad in (["--qvalue-method=storey"], ["--qvalue-method=minp"], ["--qvalue-method=efdr"], ["--descriptions=d.tsv"], ["--counter=segment-overlap"]):
        with pytest.raises(SystemExit):
            mod.buildParser().parse_args(bad)
    for argv, what in ((["--conditional=cooccurance"], "conditional"), (["--annotations-to-points=midpoint"], "annotations-to-points"),
                       (["--reference-stream"], "reference-stream")):
        with pytest.raises(NotImplementedError, match="gat-geneset.*%s" % what):
            mod.main(["gat-geneset.py"] + argv)
    with pytest.raises(ValueError, match="--gene-sets"):
        mod.main(["gat-geneset.py", "--segments=s.bed"])
    with pytest.raises(NotImplementedError, match="run on the GPU path"):
        geneset.track_geneset("t", None, [], [], ["x"], [0, 0], [], None, object(), 10)
    with pytest.raises(SystemExit) as e:
        mod.main(["gat-geneset.py", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--gene-sets" in text and "--min-term-genes" in text and "--genes" in text and "hypergeom_pvalue" in text


def test_refused_before_the_device(monkeypatch, tmp_path):
    """no samples, an unknown q-value method, too many genes: ValueError; nothing reaches the library"""
    from gat_amd import geneset
    mod = script()
    genes_file, map_file = write_cli_genes(tmp_path)
    opts, _ = mod.buildParser().parse_args(["--segments=%s" % os.path.join(CLI, "segments.bed"), "--genes=%s" % genes_file,
                                            "--gene-sets=%s" % map_file, "--workspace=%s" % os.path.join(CLI, "workspace.bed")])
    segments, annotations, workspace = geneset.build_inputs(opts)
    sets = geneset.read_gene_sets(map_file)
    ids, genes, dropped = geneset.gene_table(annotations)
    assert dropped >= 1 and len(ids) + dropped == 155 and list(sets) == ["T0", "T5", "T1", "T2", "T3", "T4", "T6"]
    terms, term_off, term_genes, unknown = geneset.term_table(sets, ids)
    assert unknown == 1 + dropped and np.diff(term_off)[terms.index("T6")] == 1 and np.diff(term_off).min() >= 1
    lines = []
    monkeypatch.setattr(geneset, "get_context", lambda: pytest.fail("the device was asked"))
    with pytest.raises(ValueError, match="num_samples"):
        geneset.run(segments, annotations, sets, workspace, geneset.make_sampler(opts), 0, random_seed=1, log=lines.append)
    assert lines == ["gat-geneset: %d genes in the workspace, %d genes without a base in it dropped" % (len(ids), dropped),
                     "gat-geneset: 7 terms, %d gene ids of the map not in the gene file ignored" % unknown]
    with pytest.raises(ValueError, match="qvalue-method"):
        geneset.run(segments, annotations, sets, workspace, geneset.make_sampler(opts), 10, qvalue_method="storey")
    monkeypatch.setattr(geneset, "MAX_GENES", 2)
    with pytest.raises(ValueError, match="genes are more than 2"):
        geneset.run(segments, annotations, sets, workspace, geneset.make_sampler(opts), 10, random_seed=1)


def test_annotation_overlap_is_the_intervals_hit():
    """what tests/test_geneset_gpu.py compares a term with: on normalized lists CounterAnnotationOverlap (the oracle's) counts
    the intervals of the track that share a base with a segment -- no midpoints, no bases"""
    from oracle import oracle as O
    from local_model import random_normalized
    r = random.Random(5)
    n = 0
    for _ in range(60):
        segs = random_normalized(r, r.choice([0, 1, 5, 30]), 600, 25)
        track = random_normalized(r, r.choice([1, 4, 40]), 600, 25)
        want = sum(1 for a, b in track if any(s < b and a < e for s, e in segs))
        assert O.counter("annotation-overlap", segs, track) == float(want)
        # ... and that is c of a term of one gene per interval
        flat = M.flatten([[[iv]] for iv in track], 1)
        assert M.counts([segs], flat, [range(len(track))])[0] == want
        n += want
    assert n > 100
