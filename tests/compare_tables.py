"""Shared by the gat-compare tests: the golden cases, the script as a module, and the field-by-field comparison of two
result tables -- text columns and pvalue / qvalue equal as strings, the %6.4f columns at most one unit of the last
printed digit apart."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "compare")
HEADERS = ["track", "annotation", "observed", "expected", "CI95low", "CI95high", "stddev", "fold", "l2fold", "pvalue", "qvalue"]
EXACT = ("track", "annotation", "pvalue", "qvalue")


def cases():
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        return json.load(f)


def script():
    spec = importlib.util.spec_from_file_location("gat_compare_cli", os.path.join(HERE, "..", "scripts", "gat-compare.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(mod, name, out_path):
    """the script on a golden case; returns (table lines it wrote, the reference's lines)"""
    case = cases()[name]
    rc = mod.main(["gat-compare.py", "--stdout=%s" % out_path] + case["args"] + [os.path.join(GOLDEN, f) for f in case["files"]])
    assert rc == 0
    got = [l for l in open(out_path) if not l.startswith("#")]
    want = open(os.path.join(GOLDEN, "expected_%s.tsv" % name)).readlines()
    return got, want


def assert_tables_match(got, want):
    assert len(got) == len(want)
    assert got[0].rstrip("\n").split("\t") == HEADERS == want[0].rstrip("\n").split("\t")
    for g_line, w_line in zip(got[1:], want[1:]):
        g, w = g_line.rstrip("\n").split("\t"), w_line.rstrip("\n").split("\t")
        assert len(g) == len(w) == len(HEADERS)
        for name, a, b in zip(HEADERS, g, w):
            if name in EXACT or a == b:
                assert a == b, (name, g_line, w_line)
            else:
                # four decimals printed: one unit of the last digit (and the representation error of the two parsed values)
                assert abs(float(a) - float(b)) <= 1e-4 + 1e-9, (name, g_line, w_line)
