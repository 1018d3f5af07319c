"""one-off sweep of the fuzz generator of tests/test_hip_parity.py over many seeds (GPU vs oracle, bit-exact), or of the
shift / global permutation edge cases of tests/test_sampler_edges_gpu.py (GPU vs tests/shift_model.py, permutation_model.py),
or of the local permutation sampler's random units (tests/local_permutation_edges.py, GPU vs local_permutation_model.py),
or of the brute-force sampler's edge cases (tests/brute_force_edges.py edge_units, GPU vs brute_force_model.py; a seed
whose model does not converge is counted and left out);
usage: tools/fuzz_sweep.py first_seed n_seeds [edge|merged|long|scan|frag|units|shift|perm|local|brute]"""
import importlib.util, os, sys, time
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
spec = importlib.util.spec_from_file_location("thp", os.path.join(root, "tests", "test_hip_parity.py"))
m = importlib.util.module_from_spec(spec)
spec.loader.exec_module(m)
spec = importlib.util.spec_from_file_location("tse", os.path.join(root, "tests", "test_sampler_edges_gpu.py"))
se = importlib.util.module_from_spec(spec)
spec.loader.exec_module(se)
from gat_amd import _lib
import random
import local_permutation_edges as LE
import brute_force_edges as BE
spec = importlib.util.spec_from_file_location("tbe", os.path.join(root, "tests", "test_sampler_brute_force_edges_gpu.py"))
be = importlib.util.module_from_spec(spec)
spec.loader.exec_module(be)


class MP(object):                      # minimal monkeypatch stand-in: the knobs go through the context's options
    def setenv(self, k, v):
        ctx.options[k] = v

    def setitem(self, d, k, v):
        d[k] = v

    def delenv(self, k):
        ctx.options.pop(k, None)

    def delitem(self, d, k):
        d.pop(k, None)


ctx = _lib.Context(0)
first, n = int(sys.argv[1]), int(sys.argv[2])
edge = len(sys.argv) > 3 and sys.argv[3] == "edge"
merged = len(sys.argv) > 3 and sys.argv[3] == "merged"
long_lists = len(sys.argv) > 3 and sys.argv[3] == "long"
scan = len(sys.argv) > 3 and sys.argv[3] == "scan"
frag = len(sys.argv) > 3 and sys.argv[3] == "frag"
units = len(sys.argv) > 3 and sys.argv[3] == "units"
shift = len(sys.argv) > 3 and sys.argv[3] == "shift"
perm = len(sys.argv) > 3 and sys.argv[3] == "perm"
local = len(sys.argv) > 3 and sys.argv[3] == "local"
brute = len(sys.argv) > 3 and sys.argv[3] == "brute"
unconverged = 0
uo = [0, 0, 0]
handed = 0
bad = 0
outcomes = {}
t0 = time.time()
for seed in range(first, first + n):
    for k in ("GAT_TEST_HUGE", "GAT_PLACE_NO_WIDE", "GAT_PLACE_NO_CM", "GAT_PLACE_SCAN_SEQ", "GAT_PLACE_SCAN_TILES", "GAT_GRID_CELL_SEGS",
              "GAT_PLACE_NO_GRID", "GAT_TAIL_NO_LONG_WS", "GAT_COUNT_VIA_CONTIGS", "GAT_MERGED_MIN_TRACKS"):       # (what a seed's test sets stays set here: MP does not undo)
        ctx.options.pop(k, None)
    if (merged or long_lists or edge) and seed % 4 >= 2:
        ctx.options["GAT_PLACE_NO_CM"] = "1"           # k_place's steps as the compiler writes them (the shapes test picks by itself)
    try:
        if shift:
            se.shift_case(ctx, seed)
        elif perm:
            se.perm_case(ctx, seed)
        elif brute:                    # the call of test_brute_fuzz[seed], for any seed
            if BE.model_units(*BE.fuzz_call(seed))[1]["unconverged"]:
                unconverged += 1
            else:
                be.brute_case(ctx, seed)
        elif local:                    # 12 random units (a third fragmented) x 3 samples: lists and words drawn
            flat = LE.units_flat(LE.random_units(random.Random(0x10CA1 + seed), 12))
            got, st = LE.device_units(ctx, flat, seed, 0, 3)
            want, wst = LE.model_units(flat, seed, 0, 3)
            assert got == want and st["n_draws"] == wst["n_draws"]
        elif units:
            r = m._units_direct_case(ctx, seed)
            uo = [uo[0] + r[0], uo[1] + r[1], uo[2] + (1 if r[2] else 0)]
        elif frag:
            handed += m._frag_ws_case(ctx, seed)
        elif scan:
            m._scan_case(ctx, seed, MP().setenv)
        elif merged:
            for k in ("GAT_MERGED_MIN_TRACKS", "GAT_COUNT_NO_MERGED", "GAT_MERGED_BLOCK"):
                ctx.options.pop(k, None)
            m.test_merged_track_index_vs_oracle(ctx, seed, MP())
        elif long_lists:
            handed += m._long_list_case(ctx, seed)
        elif edge:
            r = m._edge_case(ctx, seed)
            outcomes[r] = outcomes.get(r, 0) + 1
        else:
            m.test_fuzz_shapes_vs_oracle(ctx, seed, MP())
    except Exception as e:             # noqa: BLE001
        bad += 1
        print("seed %d: %s: %s" % (seed, type(e).__name__, str(e)[:300]), flush=True)
    if (seed - first + 1) % (100 if shift or perm or local or brute else 2000) == 0:  # (a sweep cut short by `timeout` still says how far it came)
        print("... %d seeds, %d failures, %.0f s" % (seed - first + 1, bad, time.time() - t0), flush=True)
print("%d seeds, %d failures, %.1f s %s" % (n, bad, time.time() - t0, outcomes if edge else ("units through k_tail_big: %d" % handed if long_lists else ("units finished by k_tail: %d" % handed if frag else ("candidates %d, overlaps taken off %d, problems repeated through k_contig %d" % tuple(uo) if units else ("seeds left out (the model does not converge): %d" % unconverged if brute else ""))))))
