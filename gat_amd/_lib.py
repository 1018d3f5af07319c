"""ctypes binding of libgat_mi355.so (C ABI: include/gat_mi355.h).

The library is the product's only compute path.  If it is missing, or no gfx950 device is
usable, everything here raises -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (GAT_LIB_PATH: a diagnostic build of the same library, tools/diag_sampler.sh)
LIB_PATH = os.environ.get("GAT_LIB_PATH") or os.path.join(HERE, "libgat_mi355.so")

SEG = np.dtype([("start", "<u4"), ("end", "<u4")])

COUNTER_IDS = {
    "nucleotide-overlap": 0,
    "nucleotide-density": 1,
    "segment-overlap": 2,
    "segment-midoverlap": 3,
    "annotation-overlap": 4,
    "annotation-midoverlap": 5,
}

# every symbol include/gat_mi355.h declares
SYMBOLS = [
    "gat_ctx_create", "gat_ctx_destroy", "gat_last_error", "gat_version", "gat_ctx_synchronize", "gat_ctx_stream", "gat_ctx_set_kernel_times",
    "gat_dev_alloc", "gat_dev_free", "gat_memcpy_d2h", "gat_memcpy_h2d",
    "gat_problem_create", "gat_problem_destroy", "gat_sample_and_count", "gat_sample", "gat_sample_units",
    "gat_count_lists", "gat_count_list_ranges", "gat_intersection_sizes", "gat_problem_info",
    "gat_comm_unique_id", "gat_comm_create", "gat_comm_destroy", "gat_allgather_counts", "gat_null_stats",
    "gat_sample_and_count_serial", "gat_mt19937_seed", "gat_sample_and_count_enqueue", "gat_wait",
    "gat_annotations_create", "gat_annotations_destroy", "gat_annotations_wait", "gat_list_sums", "gat_problem_rng_rows",
    "gat_isochore_split", "gat_comm_library_preloaded", "gat_ctx_set_option", "gat_ctx_get_option", "gat_compare_stats",
    "gat_call_lane_for", "gat_sample_coverage", "gat_list_metrics", "gat_sample_metrics", "gat_list_distances",
    "gat_sample_distances", "gat_minp_counts", "gat_minp_times", "gat_efdr_counts", "gat_efdr_times",
    "gat_list_bin_overlaps", "gat_sample_bin_enrichment", "gat_count_last_launch", "gat_sampler_last_launch",
    "gat_list_pair_hits", "gat_sample_pair_enrichment", "gat_list_geneset_hits", "gat_sample_geneset_enrichment",
    "gat_list_profile", "gat_sample_profile_enrichment", "gat_list_signal", "gat_sample_signal",
    "gat_null_fold_reset", "gat_null_fold", "gat_list_reldist", "gat_sample_reldist_enrichment",
    "gat_list_metagene", "gat_sample_metagene_enrichment",
]
NULL_FOLD_WORDS = 8           # GAT_NULL_FOLD_WORDS: n, sum, sumsq_lo, sumsq_hi, n_less, n_eq, min, max

MT_STATE_WORDS = 625          # GAT_MT_STATE_WORDS: 624 state words + numpy's position
# gat_problem_desc::sampler (GAT_SAMPLER_*)
SAMPLER_ANNOTATOR, SAMPLER_SEGMENTS, SAMPLER_SHIFT, SAMPLER_GLOBAL_PERMUTATION, SAMPLER_LOCAL_PERMUTATION = 0, 1, 2, 3, 4
SAMPLER_BRUTE_FORCE = 5
SAMPLER_CIRCULAR = 6
SAMPLER_UNIVERSE = 7


def mt19937_seed(seed):
    """the state numpy.random.seed(seed) leaves for an integer seed (624 words + position 624)"""
    st = np.zeros(MT_STATE_WORDS, dtype=np.uint32)
    lib().gat_mt19937_seed(int(seed) & 0xFFFFFFFF, _p(st))
    return st


COUNT_KERNELS = {0: "none", 1: "k_count_seg", 2: "k_count_swap", 3: "k_count_merged"}


COUNT_ANNO_KERNELS = {0: "none", 1: "k_count_anno_idx", 2: "k_count_anno"}


class CountReport(C.Structure):
    """gat_count_report: what the count stage launched last on a context (gat_count_last_launch)"""
    _fields_ = [
        ("kernel", C.c_int32),
        ("staged", C.c_int32),
        ("hits", C.c_int32),
        ("patch", C.c_int32),
        ("tracks_per_block", C.c_int32),
        ("samples_per_block", C.c_int32),
        ("merged_form", C.c_int32),
        ("anno_kernel", C.c_int32),
    ]

    def asdict(self):
        return dict((f, getattr(self, f)) for f, _ in self._fields_)


SAMPLER_REPORT_CLASSES = 8    # GAT_SAMPLER_REPORT_CLASSES


class SamplerClassReport(C.Structure):
    """gat_sampler_class_report: what the long-list chain and the split path were launched with for one size class"""
    _fields_ = [
        ("first", C.c_int32),
        ("merge_ccap", C.c_int32),
        ("merge_buckets", C.c_int32),
        ("merge_form", C.c_int32),
        ("consolidate_ccap", C.c_int32),
    ]


class SamplerReport(C.Structure):
    """gat_sampler_report: what the sampler stage planned for the newest batch of a call (gat_sampler_last_launch)"""
    _fields_ = [
        ("huge", C.c_int32),
        ("split", C.c_int32),
        ("long_lists", C.c_int32),
        ("merge_big", C.c_int32),
        ("tail_big", C.c_int32),
        ("resume_big", C.c_int32),
        ("long_queue", C.c_int32),
        ("resume_virtual", C.c_int32),
        ("tree", C.c_int32),
        ("big_buckets", C.c_int32),
        ("n_long", C.c_int32),
        ("sampler_variant", C.c_int32),
        ("n_classes", C.c_int32),
        ("cls", SamplerClassReport * SAMPLER_REPORT_CLASSES),
    ]

    def asdict(self):
        d = dict((f, getattr(self, f)) for f, _ in self._fields_ if f != "cls")
        d["classes"] = [dict((f, getattr(c, f)) for f, _ in SamplerClassReport._fields_)
                        for c in self.cls[:min(self.n_classes, SAMPLER_REPORT_CLASSES)]]
        return d


class GatError(RuntimeError):
    pass


class ProblemDesc(C.Structure):
    _fields_ = [
        ("n_units", C.c_int32),
        ("segs", C.c_void_p),
        ("seg_off", C.c_void_p),
        ("ws", C.c_void_p),
        ("ws_off", C.c_void_p),
        ("unit_contig", C.c_void_p),
        ("n_contigs", C.c_int32),
        ("merge_contigs", C.c_int32),
        ("n_tracks", C.c_int32),
        ("annos", C.c_void_p),
        ("anno_off", C.c_void_p),
        ("cws_nseg", C.c_void_p),
        ("bucket_size", C.c_uint32),
        ("nbuckets", C.c_int32),
        ("sampler", C.c_int32),
        ("n_anno_lists", C.c_int64),
        ("anno_end", C.c_void_p),
        ("anno_group", C.c_void_p),
        ("annotations", C.c_void_p),
        ("shift_radius", C.c_double),
        ("shift_extension", C.c_int32),
        ("brute_ntries_inner", C.c_int32),
        ("brute_ntries_outer", C.c_int32),
    ]


class AnnotationsDesc(C.Structure):
    _fields_ = [
        ("n_tracks", C.c_int32),
        ("n_contigs", C.c_int32),
        ("merge_contigs", C.c_int32),
        ("annos", C.c_void_p),
        ("anno_off", C.c_void_p),
        ("n_anno_lists", C.c_int64),
        ("anno_end", C.c_void_p),
        ("anno_group", C.c_void_p),
        ("mean_segment_length", C.c_double),
        ("flags", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("ms_sampler", C.c_float),
        ("ms_contig", C.c_float),
        ("ms_count", C.c_float),
        ("ms_total", C.c_float),
        ("n_placed", C.c_int64),
        ("n_draws", C.c_int64),
        ("n_sampled_segments", C.c_int64),
        ("n_unsuccessful", C.c_int64),
        ("n_retried", C.c_int64),
        ("n_full_units", C.c_int64),
        ("ms_count_main", C.c_float),
        ("ms_rng", C.c_float),
        ("ms_place", C.c_float),
        ("ms_merge", C.c_float),
        ("ms_tail", C.c_float),
        ("count_kernel", C.c_int32),
        ("ms_ktail", C.c_float),
        ("ms_finalize", C.c_float),
        ("n_tail_units", C.c_int64),
        ("lists_from_records", C.c_int64),
        ("n_index_entries", C.c_int64),
        ("n_index_lookups", C.c_int64),
        ("n_batches", C.c_int64),
        ("merged_form", C.c_int64),
        ("n_resumed_units", C.c_int64),
        ("n_straddle_candidates", C.c_int64),
        ("n_unit_overlaps", C.c_int64),
        ("kernel_times", C.c_int64),
        ("n_queued_units", C.c_int64),
        ("n_empty_windows", C.c_int64),
        ("n_restarts", C.c_int64),
        ("n_unconverged", C.c_int64),
    ]

    def asdict(self):
        return dict((f, getattr(self, f)) for f, _ in self._fields_)


# gat_compare_stats(ctx, a_dev, n_rows_a, b_dev, n_rows_b, n_samples, ia, ib, n_pairs, obs_a, obs_b, delta, pseudo_count,
#                   lo_index, hi_index, out): include/gat_mi355.h
COMPARE_STATS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_void_p]

_LIB = None


def lib():
    """load libgat_mi355.so; raises GatError if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise GatError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); gat_amd has no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    L.gat_ctx_create.restype = C.c_int
    L.gat_ctx_create.argtypes = [C.POINTER(vp), C.c_int, vp]
    L.gat_ctx_destroy.restype = None
    L.gat_ctx_destroy.argtypes = [vp]
    L.gat_last_error.restype = C.c_char_p
    L.gat_last_error.argtypes = [vp]
    L.gat_version.restype = C.c_char_p
    L.gat_version.argtypes = []
    L.gat_ctx_synchronize.restype = C.c_int
    L.gat_ctx_synchronize.argtypes = [vp]
    L.gat_ctx_stream.restype = vp
    L.gat_ctx_stream.argtypes = [vp]
    L.gat_ctx_set_kernel_times.restype = C.c_int
    L.gat_ctx_set_kernel_times.argtypes = [vp, C.c_int]
    L.gat_dev_alloc.restype = C.c_int
    L.gat_dev_alloc.argtypes = [vp, C.POINTER(vp), C.c_size_t]
    L.gat_dev_free.restype = C.c_int
    L.gat_dev_free.argtypes = [vp, vp]
    L.gat_memcpy_d2h.restype = C.c_int
    L.gat_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.gat_memcpy_h2d.restype = C.c_int
    L.gat_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.gat_problem_create.restype = C.c_int
    L.gat_problem_create.argtypes = [vp, C.POINTER(ProblemDesc), C.POINTER(vp)]
    L.gat_problem_destroy.restype = None
    L.gat_problem_destroy.argtypes = [vp]
    L.gat_annotations_create.restype = C.c_int
    L.gat_annotations_create.argtypes = [vp, C.POINTER(AnnotationsDesc), C.POINTER(vp)]
    L.gat_annotations_wait.restype = C.c_int
    L.gat_annotations_wait.argtypes = [vp, vp]
    L.gat_annotations_destroy.restype = None
    L.gat_annotations_destroy.argtypes = [vp]
    L.gat_sample_and_count.restype = C.c_int
    L.gat_sample_and_count.argtypes = [vp, vp, vp, C.c_int, u32, i64, i64, vp, C.POINTER(Stats)]
    L.gat_sample_and_count_enqueue.restype = C.c_int
    L.gat_sample_and_count_enqueue.argtypes = [vp, vp, vp, C.c_int, u32, i64, i64, vp]
    L.gat_wait.restype = C.c_int
    L.gat_wait.argtypes = [vp, vp, C.POINTER(Stats)]
    L.gat_sample_and_count_serial.restype = C.c_int
    L.gat_sample_and_count_serial.argtypes = [vp, vp, vp, C.c_int, vp, i64, vp, C.POINTER(Stats)]
    L.gat_mt19937_seed.restype = None
    L.gat_mt19937_seed.argtypes = [u32, vp]
    L.gat_sample.restype = C.c_int
    L.gat_sample.argtypes = [vp, vp, u32, i64, i64, vp, i64, vp, C.POINTER(Stats)]
    L.gat_sample_units.restype = C.c_int
    L.gat_sample_units.argtypes = [vp, vp, u32, i64, i64, vp, i64, vp, C.POINTER(Stats)]
    L.gat_sample_coverage.restype = C.c_int
    L.gat_sample_coverage.argtypes = [vp, vp, u32, i64, i64, i64, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.gat_list_metrics.restype = C.c_int
    L.gat_list_metrics.argtypes = [vp, vp, vp, i64, vp, vp, i32, vp]
    L.gat_sample_metrics.restype = C.c_int
    L.gat_sample_metrics.argtypes = [vp, vp, u32, i64, i64, vp, vp, vp, C.POINTER(Stats)]
    L.gat_list_distances.restype = C.c_int
    L.gat_list_distances.argtypes = [vp, vp, vp, i64, vp, vp, i32, i32, C.c_int, i64, vp]
    L.gat_sample_distances.restype = C.c_int
    L.gat_sample_distances.argtypes = [vp, vp, u32, i64, i64, vp, vp, i32, C.c_int, i64, vp, C.POINTER(Stats)]
    L.gat_list_signal.restype = C.c_int
    L.gat_list_signal.argtypes = [vp, vp, vp, i64, vp, vp, vp, i32, i32, vp]
    L.gat_sample_signal.restype = C.c_int
    L.gat_sample_signal.argtypes = [vp, vp, u32, i64, i64, vp, vp, vp, i32, vp, C.POINTER(Stats)]
    L.gat_list_bin_overlaps.restype = C.c_int
    L.gat_list_bin_overlaps.argtypes = [vp, vp, vp, i64, vp, vp, i32, i32, i64, vp, vp]
    L.gat_sample_bin_enrichment.restype = C.c_int
    L.gat_sample_bin_enrichment.argtypes = [vp, vp, u32, i64, i64, vp, vp, i32, i64, vp, vp, vp, C.POINTER(Stats)]
    L.gat_list_pair_hits.restype = C.c_int
    L.gat_list_pair_hits.argtypes = [vp, vp, vp, i64, vp, vp, i32, i32, vp]
    L.gat_sample_pair_enrichment.restype = C.c_int
    L.gat_sample_pair_enrichment.argtypes = [vp, vp, u32, i64, i64, vp, vp, i32, vp, vp, C.POINTER(Stats)]
    L.gat_list_geneset_hits.restype = C.c_int
    L.gat_list_geneset_hits.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, i32, i32, vp]
    L.gat_sample_geneset_enrichment.restype = C.c_int
    L.gat_sample_geneset_enrichment.argtypes = [vp, vp, u32, i64, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, C.POINTER(Stats)]
    L.gat_list_profile.restype = C.c_int
    L.gat_list_profile.argtypes = [vp, vp, vp, i64, vp, vp, vp, i32, i32, i64, i32, C.c_int, vp]
    L.gat_sample_profile_enrichment.restype = C.c_int
    L.gat_sample_profile_enrichment.argtypes = [vp, vp, u32, i64, i64, vp, vp, vp, i32, i64, i32, C.c_int, vp, vp, C.POINTER(Stats)]
    L.gat_list_reldist.restype = C.c_int
    L.gat_list_reldist.argtypes = [vp, vp, vp, i64, vp, vp, i32, i32, i32, vp]
    L.gat_sample_reldist_enrichment.restype = C.c_int
    L.gat_sample_reldist_enrichment.argtypes = [vp, vp, u32, i64, i64, vp, vp, i32, i32, vp, vp, C.POINTER(Stats)]
    L.gat_list_metagene.restype = C.c_int
    L.gat_list_metagene.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i64, C.c_int, vp]
    L.gat_sample_metagene_enrichment.restype = C.c_int
    L.gat_sample_metagene_enrichment.argtypes = [vp, vp, u32, i64, i64, vp, vp, vp, vp, i32, i32, i32, i64, C.c_int, vp, vp, C.POINTER(Stats)]
    L.gat_count_lists.restype = C.c_int
    L.gat_count_lists.argtypes = [vp, vp, C.c_int, vp, vp, i64, vp, vp, i32, vp, i32, vp]
    L.gat_count_list_ranges.restype = C.c_int
    L.gat_count_list_ranges.argtypes = [vp, vp, C.c_int, vp, vp, i64, vp, vp, vp, i32, vp, i32, vp]
    L.gat_count_last_launch.restype = C.c_int
    L.gat_count_last_launch.argtypes = [vp, C.POINTER(CountReport)]
    L.gat_sampler_last_launch.restype = C.c_int
    L.gat_sampler_last_launch.argtypes = [vp, C.POINTER(SamplerReport)]
    L.gat_call_lane_for.restype = C.c_int
    L.gat_call_lane_for.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.gat_intersection_sizes.restype = C.c_int
    L.gat_intersection_sizes.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, vp]
    L.gat_problem_rng_rows.restype = i64
    L.gat_problem_rng_rows.argtypes = [vp]
    L.gat_list_sums.restype = C.c_int
    L.gat_list_sums.argtypes = [vp, vp, vp, i64, vp]
    L.gat_isochore_split.restype = C.c_int
    L.gat_isochore_split.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, i32, i32, vp, vp, vp]
    L.gat_problem_info.restype = C.c_int
    L.gat_problem_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.gat_null_stats.restype = C.c_int
    L.gat_null_stats.argtypes = [vp, vp, i64, i64, vp, vp, i64, i64, vp]
    L.gat_null_fold_reset.restype = C.c_int
    L.gat_null_fold_reset.argtypes = [vp, vp, i64]
    L.gat_null_fold.restype = C.c_int
    L.gat_null_fold.argtypes = [vp, vp, i64, i64, i64, vp, vp]
    L.gat_compare_stats.restype = C.c_int
    L.gat_compare_stats.argtypes = COMPARE_STATS_ARGTYPES
    L.gat_minp_counts.restype = C.c_int
    L.gat_minp_counts.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp]
    L.gat_minp_times.restype = C.c_int
    L.gat_minp_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.gat_efdr_counts.restype = C.c_int
    L.gat_efdr_counts.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, C.c_int32, vp, vp]
    L.gat_efdr_times.restype = C.c_int
    L.gat_efdr_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.gat_comm_unique_id.restype = C.c_int
    L.gat_comm_unique_id.argtypes = [vp]
    L.gat_comm_library_preloaded.restype = C.c_int
    L.gat_comm_library_preloaded.argtypes = []
    L.gat_ctx_set_option.restype = C.c_int
    L.gat_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.gat_ctx_get_option.restype = C.c_char_p
    L.gat_ctx_get_option.argtypes = [vp, C.c_char_p]
    L.gat_comm_create.restype = C.c_int
    L.gat_comm_create.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, vp]
    L.gat_comm_destroy.restype = None
    L.gat_comm_destroy.argtypes = [vp]
    L.gat_allgather_counts.restype = C.c_int
    L.gat_allgather_counts.argtypes = [vp, vp, vp, vp, i64]
    _LIB = L
    return L


_ERRORS = {-1: ValueError, -2: AssertionError, -3: GatError, -4: MemoryError, -5: GatError, -6: ValueError}


def _check(rc, ctx=None):
    if rc == 0:
        return
    msg = lib().gat_last_error(ctx).decode("utf-8", "replace")
    raise _ERRORS.get(rc, GatError)("gat_mi355 error %d: %s" % (rc, msg))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class _Options(object):
    """a context's tuning / testing knobs (gat_ctx_set_option) as a mapping: options["GAT_X"] = "1" sets, del / pop go back to
    the process's value (the environment as the library first saw it), "" means "not set whatever the environment says".
    pytest's monkeypatch.setitem(ctx.options, key, value) undoes itself."""

    def __init__(self, ctx):
        self._ctx = ctx
        self._mine = {}

    def __setitem__(self, key, value):
        _check(lib().gat_ctx_set_option(self._ctx._h, key.encode(), str(value).encode()), self._ctx._h)
        self._mine[key] = str(value)

    def __delitem__(self, key):
        _check(lib().gat_ctx_set_option(self._ctx._h, key.encode(), None), self._ctx._h)
        del self._mine[key]

    def __getitem__(self, key):
        return self._mine[key]                      # (KeyError: not set on this context -- what monkeypatch.setitem asks)

    def __contains__(self, key):
        return key in self._mine

    def get(self, key, default=None):
        """the value in force: this context's, else the process's; None: not set"""
        v = lib().gat_ctx_get_option(self._ctx._h, key.encode())
        return v.decode() if v is not None else default

    def pop(self, key, default=None):
        if key in self._mine:
            v = self._mine[key]
            del self[key]
            return v
        return default

    def update(self, **kw):
        for k, v in kw.items():
            self[k] = v


class Context(object):
    """one HIP device + stream (gat_ctx)."""

    def __init__(self, device=0, stream=None):
        """stream: a hipStream_t handle to run on (e.g. torch.cuda.Stream(...).cuda_stream); None: the context makes a
        private non-blocking stream; 0 -- the handle torch reports for its DEFAULT stream -- means that stream (it is
        passed on as hipStreamLegacy: a NULL handle is the C ABI's "make a private stream")."""
        self._h = C.c_void_p()
        if stream is None:
            handle = None
        else:
            handle = C.c_void_p(int(stream) if int(stream) != 0 else 1)      # hipStreamLegacy == (hipStream_t)1
        _check(lib().gat_ctx_create(C.byref(self._h), int(device), handle))
        self.device = device
        self.options = _Options(self)           # the knobs (GAT_*): ctx.options["GAT_NO_SPLIT"] = "1"

    def close(self):
        if self._h:
            lib().gat_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().gat_ctx_synchronize(self._h), self._h)

    def stream_handle(self):
        """the hipStream_t the context enqueues on, as an integer (torch.cuda.ExternalStream(handle) orders torch's work
        against the library's with events, no device-wide synchronisation)"""
        return int(lib().gat_ctx_stream(self._h) or 0)

    def set_kernel_times(self, on):
        """per-kernel device times in the statistics of a call (ms_rng, ms_place, ...): off by default, an event behind
        every kernel costs a call 50-60 us"""
        _check(lib().gat_ctx_set_kernel_times(self._h, 1 if on else 0), self._h)

    def alloc(self, nbytes):
        p = C.c_void_p()
        _check(lib().gat_dev_alloc(self._h, C.byref(p), nbytes), self._h)
        return p.value

    def free(self, ptr):
        _check(lib().gat_dev_free(self._h, C.c_void_p(ptr)), self._h)

    def d2h(self, host_array, dev_ptr):
        _check(lib().gat_memcpy_d2h(self._h, _p(host_array), C.c_void_p(dev_ptr), host_array.nbytes), self._h)

    def null_stats(self, counts_dev_ptr, n_rows, n_samples, is_double, vals):
        """per row of a device count matrix: (mean, std, lower95 value, upper95 value, n < val, n == val) -- what
        AnnotatorResult reads off a null distribution (gat/Engine.pyx:1635-1718), numpy.mean / numpy.std bit for bit."""
        l = int(n_samples)  # noqa: E741
        offset = int(0.05 * l)
        lo_i, hi_i = (min(offset, l - 1), max(l - offset, 0)) if offset > 0 else (0, l - 1)      # gat/Engine.pyx:1689-1696
        hi_i = min(hi_i, l - 1)
        is_double = np.ascontiguousarray(is_double, dtype=np.uint8)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        out = np.zeros((int(n_rows), 8), dtype=np.float64)
        _check(lib().gat_null_stats(self._h, C.c_void_p(counts_dev_ptr), int(n_rows), l, _p(is_double), _p(vals), lo_i, hi_i,
                                    _p(out)), self._h)
        out[:, 1] = np.sqrt(out[:, 1] / l)                # numpy.std's last two steps (sum of squares from the device)
        return out

    def null_fold_reset(self, words_dev_ptr, n_rows):
        """the eight words (NULL_FOLD_WORDS) of n_rows rows before anything is folded into them: zeros, min = 2^64 - 1"""
        _check(lib().gat_null_fold_reset(self._h, C.c_void_p(words_dev_ptr), int(n_rows)), self._h)

    def null_fold(self, counts_dev_ptr, n_rows, n_samples, row_stride, vals, words_dev_ptr):
        """a round of a device count matrix -- the first n_samples slots of rows row_stride slots apart -- added to the rows'
        words (gat_null_fold): n, sum, the 128-bit sum of squares, the samples below and equal to vals[row], min, max; exact
        integers, whatever the cut into rounds.  Returns when the kernel has completed."""
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert len(vals) == int(n_rows)
        _check(lib().gat_null_fold(self._h, C.c_void_p(counts_dev_ptr), int(n_rows), int(n_samples), int(row_stride), _p(vals),
                                   C.c_void_p(words_dev_ptr)), self._h)

    def null_fold_words(self, words_dev_ptr, n_rows):
        """the words read back: n_rows tuples of NULL_FOLD_WORDS Python ints"""
        w = np.zeros((int(n_rows), NULL_FOLD_WORDS), dtype=np.uint64)
        if n_rows:
            self.d2h(w, words_dev_ptr)
        return [tuple(int(x) for x in row) for row in w.tolist()]

    def h2d(self, dev_ptr, host_array):
        host_array = np.ascontiguousarray(host_array)
        _check(lib().gat_memcpy_h2d(self._h, C.c_void_p(dev_ptr), _p(host_array), host_array.nbytes), self._h)

    def compare_stats(self, a_dev_ptr, n_rows_a, b_dev_ptr, n_rows_b, n_samples, ia, ib, obs_a, obs_b, delta, pseudo_count):
        """per pair (ia[p], ib[p]) of rows of two device float64 matrices: null_stats' row of the pair's transformed samples
        log((obs_a / (a + pseudo_count) + 0.0001) / (obs_b / (b + pseudo_count) + 0.0001)) + delta with val = delta, and in
        column 6 how many of those samples are not finite (gat_compare_stats; the rows stay on the device)."""
        l = int(n_samples)  # noqa: E741
        offset = int(0.05 * l)
        lo_i, hi_i = (min(offset, l - 1), max(l - offset, 0)) if offset > 0 else (0, l - 1)      # gat/Engine.pyx:1689-1696
        hi_i = min(hi_i, l - 1)
        ia = np.ascontiguousarray(ia, dtype=np.int32)
        ib = np.ascontiguousarray(ib, dtype=np.int32)
        obs_a, obs_b, delta = (np.ascontiguousarray(x, dtype=np.float64) for x in (obs_a, obs_b, delta))
        n = len(ia)
        assert len(ib) == len(obs_a) == len(obs_b) == len(delta) == n
        out = np.zeros((n, 8), dtype=np.float64)
        _check(lib().gat_compare_stats(self._h, C.c_void_p(a_dev_ptr), int(n_rows_a), C.c_void_p(b_dev_ptr), int(n_rows_b), l,
                                       _p(ia), _p(ib), n, _p(obs_a), _p(obs_b), _p(delta), float(pseudo_count), lo_i, hi_i,
                                       _p(out)), self._h)
        with np.errstate(invalid="ignore"):
            out[:, 1] = np.sqrt(out[:, 1] / l)                # numpy.std's last two steps
        return out

    def minp_counts(self, counts_dev_ptr, n_rows, n_samples, is_double, means, k_obs):
        """step-down minP on a device count matrix (gat_minp_counts): per row, in the order of the rows, the number of samples
        whose running minimum over the rows at and behind it in (k_obs, index) order is at most the row's k_obs -- int64,
        before the running maximum.  means: each row's `expected`; k_obs: its p-value times n_samples."""
        n = int(n_rows)
        is_double = np.ascontiguousarray(is_double, dtype=np.uint8)
        means = np.ascontiguousarray(means, dtype=np.float64)
        k_obs = np.ascontiguousarray(k_obs, dtype=np.int32)
        assert len(is_double) == len(means) == len(k_obs) == max(n, 0)
        out = np.zeros(max(n, 0), dtype=np.int64)
        _check(lib().gat_minp_counts(self._h, C.c_void_p(counts_dev_ptr), n, int(n_samples), _p(is_double), _p(means), _p(k_obs),
                                     _p(out)), self._h)
        return out

    def minp_times(self):
        """(ms in k_minp_rank, ms in k_minp_step) of the last minp_counts; zeros unless set_kernel_times(True)"""
        a, b = C.c_float(), C.c_float()
        _check(lib().gat_minp_times(self._h, C.byref(a), C.byref(b)), self._h)
        return a.value, b.value

    def efdr_counts(self, counts_dev_ptr, n_rows, n_samples, is_double, means, k_obs, levels=()):
        """the resampling-based FDR's counts on a device count matrix (gat_efdr_counts): (v, per_sample) -- v[r] = (V_1, V_0) at
        the row's k_obs, int64, in the order of the rows: the samples of ALL rows scoring at or below it, by the tail they lie
        in (1: above their row's mean); per_sample[l] = (N_1, N_0), int32 [2][n_samples]: per sample the rows scoring at or
        below levels[l] (at most 8 levels).  means, k_obs: as for minp_counts."""
        n = int(n_rows)
        is_double = np.ascontiguousarray(is_double, dtype=np.uint8)
        means = np.ascontiguousarray(means, dtype=np.float64)
        k_obs = np.ascontiguousarray(k_obs, dtype=np.int32)
        levels = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
        assert len(is_double) == len(means) == len(k_obs) == max(n, 0)
        v = np.zeros((max(n, 0), 2), dtype=np.int64)
        per_sample = np.zeros((len(levels), 2, max(int(n_samples), 0)), dtype=np.int32)
        _check(lib().gat_efdr_counts(self._h, C.c_void_p(counts_dev_ptr), n, int(n_samples), _p(is_double), _p(means), _p(k_obs),
                                     _p(levels) if len(levels) else None, len(levels), _p(v),
                                     _p(per_sample) if len(levels) else None), self._h)
        return v, per_sample

    def efdr_times(self):
        """(ms in k_minp_rank, ms in k_efdr) of the last efdr_counts; zeros unless set_kernel_times(True)"""
        a, b = C.c_float(), C.c_float()
        _check(lib().gat_efdr_times(self._h, C.byref(a), C.byref(b)), self._h)
        return a.value, b.value

    def count_lists(self, counters, lists, list_off, n_lists, annos, anno_off, n_tracks, ws_nseg, n_groups, anno_end=None):
        """Counter*(list, annotation, workspace) for n_lists x n_groups lists (observed counts).  anno_end given: the
        annotation lists are the ranges annos[anno_off[l]:anno_end[l]] (gat_count_list_ranges), else anno_off is a CSR."""
        ids = np.array([COUNTER_IDS[c] for c in counters], dtype=np.int32)
        lists = np.ascontiguousarray(lists, dtype=SEG)
        annos = np.ascontiguousarray(annos, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
        ws_nseg = np.ascontiguousarray(ws_nseg, dtype=np.int64)
        out = np.zeros((len(ids), n_tracks, n_lists), dtype=np.int64)
        if anno_end is None:
            _check(lib().gat_count_lists(self._h, _p(ids), len(ids), _p(lists), _p(list_off), n_lists, _p(annos),
                                         _p(anno_off), n_tracks, _p(ws_nseg), n_groups, _p(out)), self._h)
        else:
            anno_end = np.ascontiguousarray(anno_end, dtype=np.int64)
            assert len(anno_off) == len(anno_end) == n_tracks * n_groups
            _check(lib().gat_count_list_ranges(self._h, _p(ids), len(ids), _p(lists), _p(list_off), n_lists, _p(annos),
                                               _p(anno_off), _p(anno_end), n_tracks, _p(ws_nseg), n_groups, _p(out)), self._h)
        return [out[k].view(np.float64).copy() if c == "nucleotide-density" else out[k].copy()
                for k, c in enumerate(counters)]

    def count_report(self):
        """what the count stage launched last on this context, as a dict of gat_count_report's fields: the newest batch of a
        sample_and_count, or the last list of a count_lists (COUNT_KERNELS / COUNT_ANNO_KERNELS name the kernels)"""
        r = CountReport()
        _check(lib().gat_count_last_launch(self._h, C.byref(r)), self._h)
        return r.asdict()

    def sampler_report(self):
        """what the sampler stage planned for the newest batch of this context's last sampling call, as a dict of
        gat_sampler_report's fields; "classes": one dict per size class of the launch order (the first SAMPLER_REPORT_CLASSES)"""
        r = SamplerReport()
        _check(lib().gat_sampler_last_launch(self._h, C.byref(r)), self._h)
        return r.asdict()

    def list_bin_overlaps(self, lists, list_off, n_lists, annos, anno_off, n_tracks, n_groups, bin_size, n_bins):
        """the bases every one of n_lists x n_groups caller-provided normalized lists -- list l of group g is
        lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]] -- shares with every one of n_tracks x n_groups
        normalized annotation lists, track t of group g at index t * n_groups + g, per bin of bin_size bases
        (gat_list_bin_overlaps): n_bins[g] bins for group g.  Returns (values, bin_off): int64 [n_lists, n_tracks, total_bins],
        group g's bins at [bin_off[g], bin_off[g + 1])."""
        lists = np.ascontiguousarray(lists, dtype=SEG)
        annos = np.ascontiguousarray(annos, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
        n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
        assert len(list_off) == n_lists * n_groups + 1 and len(anno_off) == n_tracks * n_groups + 1
        bin_off = _bin_offsets(n_bins, n_groups)
        out = np.zeros((n_lists, n_tracks, max(0, int(bin_off[-1]))), dtype=np.int64)
        _check(lib().gat_list_bin_overlaps(self._h, _p(lists), _p(list_off), n_lists, _p(annos), _p(anno_off), n_tracks, n_groups,
                                           int(bin_size), _p(bin_off), _p(out)), self._h)
        return out, bin_off

    def list_pair_hits(self, lists, list_off, n_lists, annos, anno_off, n_tracks, n_groups):
        """how many segments of every one of n_lists caller-provided lists -- list l of group g is
        lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]], in any order -- hit both tracks of every pair
        (i, j), i <= j, of n_tracks x n_groups normalized annotation lists, track t of group g at index t * n_groups + g
        (gat_list_pair_hits).  Returns int64 [n_lists, P], P = n_tracks * (n_tracks + 1) / 2, pair (i, j) at
        i * n_tracks - i * (i - 1) / 2 + (j - i)."""
        lists = np.ascontiguousarray(lists, dtype=SEG)
        annos = np.ascontiguousarray(annos, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
        n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
        assert len(list_off) == n_lists * n_groups + 1 and len(anno_off) == n_tracks * n_groups + 1
        out = np.zeros((n_lists, pair_count(n_tracks)), dtype=np.int64)
        _check(lib().gat_list_pair_hits(self._h, _p(lists), _p(list_off), n_lists, _p(annos), _p(anno_off), n_tracks, n_groups,
                                        _p(out)), self._h)
        return out

    def list_geneset_hits(self, lists, list_off, n_lists, pieces, piece_off, member_off, members, n_genes, term_off, term_genes,
                          n_terms, n_groups):
        """c(L, t) = the genes of term t hit by any segment of list L, for every one of n_lists caller-provided lists -- list l
        of group g is lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]], in any order -- and n_terms terms
        (gat_list_geneset_hits): pieces / piece_off the genes' pieces per group, member_off / members the genes that cover
        every piece, term_off / term_genes the genes of every term.  Returns int64 [n_lists, n_terms]."""
        lists = np.ascontiguousarray(lists, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        n_lists, n_genes, n_terms, n_groups = int(n_lists), int(n_genes), int(n_terms), int(n_groups)
        assert len(list_off) == n_lists * n_groups + 1
        g = _geneset_arrays(pieces, piece_off, member_off, members, term_off, term_genes, n_terms, n_groups)
        out = np.zeros((n_lists, max(0, n_terms)), dtype=np.int64)
        _check(lib().gat_list_geneset_hits(self._h, _p(lists), _p(list_off), n_lists, _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), n_genes,
                                           _p(g[4]), _p(g[5]), n_terms, n_groups, _p(out)), self._h)
        return out

    def list_profile(self, lists, list_off, n_lists, anchor_pos, anchor_minus, anchor_off, n_tracks, n_groups, bin_size, half_bins,
                     mode=0):
        """the profile of every one of n_lists x n_groups caller-provided normalized lists -- list l of group g is
        lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]] -- around the anchors of n_tracks tracks, track t of
        group g at anchor_pos / anchor_minus[anchor_off[t * n_groups + g]:anchor_off[t * n_groups + g + 1]], in 2 * half_bins
        offset bins of bin_size bases (gat_list_profile; mode: PROFILE_BASES or PROFILE_MIDPOINTS).  Returns int64
        [n_lists, n_tracks, 2 * half_bins]."""
        lists = np.ascontiguousarray(lists, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
        assert len(list_off) == n_lists * n_groups + 1
        pos, minus, anchor_off = _profile_arrays(anchor_pos, anchor_minus, anchor_off, n_tracks, n_groups)
        out = np.zeros((n_lists, n_tracks, profile_bins(half_bins)), dtype=np.int64)
        _check(lib().gat_list_profile(self._h, _p(lists), _p(list_off), n_lists, _p(pos), _p(minus), _p(anchor_off), n_tracks, n_groups,
                                      int(bin_size), int(half_bins), int(mode), _p(out)), self._h)
        return out

    def list_reldist(self, lists, list_off, n_lists, point_pos, point_off, n_tracks, n_groups, n_bins):
        """the relative distances of every one of n_lists x n_groups caller-provided lists (any lists: every segment counts
        on its own) -- list l of group g is lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]] -- to the points
        of n_tracks tracks, track t of group g at point_pos[point_off[t * n_groups + g]:point_off[t * n_groups + g + 1]],
        strictly ascending (gat_list_reldist).  Returns int64 [n_lists, n_tracks, n_bins + RELDIST_EXTRA]: the bins, then
        area (parts per million), inside, outside."""
        lists = np.ascontiguousarray(lists, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
        assert len(list_off) == n_lists * n_groups + 1
        pos, point_off = _reldist_arrays(point_pos, point_off, n_tracks, n_groups)
        out = np.zeros((n_lists, n_tracks, reldist_values(n_bins)), dtype=np.int64)
        _check(lib().gat_list_reldist(self._h, _p(lists), _p(list_off), n_lists, _p(pos), _p(point_off), n_tracks, n_groups,
                                      int(n_bins), _p(out)), self._h)
        return out

    def list_metagene(self, lists, list_off, n_lists, feat_start, feat_end, feat_minus, feat_off, n_tracks, n_groups, body_bins,
                      flank_bins, flank_bin_size, mode=0):
        """the metagene of every one of n_lists x n_groups caller-provided normalized lists -- list l of group g is
        lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]] -- along the features of n_tracks tracks, track t of
        group g at feat_start / feat_end / feat_minus[feat_off[t * n_groups + g]:feat_off[t * n_groups + g + 1]], ascending
        by (start, end, minus): flank_bins bins of flank_bin_size bases upstream, body_bins scaled bins over the feature,
        flank_bins downstream (gat_list_metagene; mode: METAGENE_BASES or METAGENE_MIDPOINTS).  Returns int64
        [n_lists, n_tracks, 2 * flank_bins + body_bins]."""
        lists = np.ascontiguousarray(lists, dtype=SEG)
        list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
        assert len(list_off) == n_lists * n_groups + 1
        fs, fe, minus, feat_off = _metagene_arrays(feat_start, feat_end, feat_minus, feat_off, n_tracks, n_groups)
        out = np.zeros((n_lists, n_tracks, metagene_bins(body_bins, flank_bins)), dtype=np.int64)
        _check(lib().gat_list_metagene(self._h, _p(lists), _p(list_off), n_lists, _p(fs), _p(fe), _p(minus), _p(feat_off), n_tracks,
                                       n_groups, int(body_bins), int(flank_bins), int(flank_bin_size), int(mode), _p(out)), self._h)
        return out


NULL_WORDS = ("n_pos", "sum", "sumsq", "n_less", "n_eq")      # the sampled null of one cell against obs: include/gat_mi355.h
# GAT_LOCAL_WORDS, GAT_PAIR_WORDS, GAT_GENESET_WORDS, GAT_PROFILE_WORDS, GAT_RELDIST_WORDS, GAT_METAGENE_WORDS
LOCAL_WORDS = PAIR_WORDS = GENESET_WORDS = PROFILE_WORDS = RELDIST_WORDS = METAGENE_WORDS = NULL_WORDS
PAIR_MAX_TRACKS = 2048        # GAT_PAIR_MAX_TRACKS
PROFILE_MAX_BINS = 1024       # GAT_PROFILE_MAX_BINS
PROFILE_BASES, PROFILE_MIDPOINTS = 0, 1       # GAT_PROFILE_BASES, GAT_PROFILE_MIDPOINTS
RELDIST_MAX_BINS = 1024       # GAT_RELDIST_MAX_BINS
RELDIST_EXTRA = 3             # GAT_RELDIST_EXTRA: area, inside, outside behind the bins
RELDIST_AREA_SCALE = 10 ** 6  # GAT_RELDIST_AREA_SCALE
METAGENE_MAX_BINS = 1024      # GAT_METAGENE_MAX_BINS
METAGENE_BASES, METAGENE_MIDPOINTS = 0, 1     # GAT_METAGENE_BASES, GAT_METAGENE_MIDPOINTS


def profile_bins(half_bins):
    """the bins of a profile (0 where half_bins is out of range: the library refuses the call)"""
    return 2 * int(half_bins) if 1 <= int(half_bins) <= PROFILE_MAX_BINS // 2 else 0


def _profile_arrays(anchor_pos, anchor_minus, anchor_off, n_tracks, n_groups):
    """the anchor arguments of the two profile calls as the library takes them"""
    pos = np.ascontiguousarray(anchor_pos, dtype=np.uint32)
    minus = np.ascontiguousarray(anchor_minus, dtype=np.uint8)
    anchor_off = np.ascontiguousarray(anchor_off, dtype=np.int64)
    assert len(anchor_off) == max(0, n_tracks) * max(0, n_groups) + 1 and len(pos) == len(minus)
    return pos, minus, anchor_off


def reldist_values(n_bins):
    """the values of a (list, track) of the relative distance calls (0 where n_bins is out of range: the library refuses the call)"""
    return int(n_bins) + RELDIST_EXTRA if 1 <= int(n_bins) <= RELDIST_MAX_BINS else 0


def _reldist_arrays(point_pos, point_off, n_tracks, n_groups):
    """the point arguments of the two relative distance calls as the library takes them"""
    pos = np.ascontiguousarray(point_pos, dtype=np.uint32)
    point_off = np.ascontiguousarray(point_off, dtype=np.int64)
    assert len(point_off) == max(0, n_tracks) * max(0, n_groups) + 1
    return pos, point_off


def metagene_bins(body_bins, flank_bins):
    """the bins of a metagene (0 where the two are out of range: the library refuses the call)"""
    body_bins, flank_bins = int(body_bins), int(flank_bins)
    return 2 * flank_bins + body_bins if body_bins >= 1 and flank_bins >= 0 and 2 * flank_bins + body_bins <= METAGENE_MAX_BINS else 0


def _metagene_arrays(feat_start, feat_end, feat_minus, feat_off, n_tracks, n_groups):
    """the feature arguments of the two metagene calls as the library takes them"""
    fs = np.ascontiguousarray(feat_start, dtype=np.uint32)
    fe = np.ascontiguousarray(feat_end, dtype=np.uint32)
    minus = np.ascontiguousarray(feat_minus, dtype=np.uint8)
    feat_off = np.ascontiguousarray(feat_off, dtype=np.int64)
    assert len(feat_off) == max(0, n_tracks) * max(0, n_groups) + 1 and len(fs) == len(fe) == len(minus)
    return fs, fe, minus, feat_off


def pair_count(n_tracks):
    """the pairs (i, j), i <= j, of n_tracks tracks (0 where n_tracks is out of range: the library refuses the call)"""
    return n_tracks * (n_tracks + 1) // 2 if 0 <= n_tracks <= PAIR_MAX_TRACKS else 0


def _geneset_arrays(pieces, piece_off, member_off, members, term_off, term_genes, n_terms, n_groups):
    """the gene and term arguments of the two geneset calls as the library takes them"""
    pieces = np.ascontiguousarray(pieces, dtype=SEG)
    piece_off, member_off, term_off = (np.ascontiguousarray(x, dtype=np.int64) for x in (piece_off, member_off, term_off))
    members, term_genes = (np.ascontiguousarray(x, dtype=np.int32) for x in (members, term_genes))
    assert len(piece_off) == max(0, n_groups) + 1 and len(term_off) == max(0, n_terms) + 1
    assert len(member_off) == max(0, int(piece_off[-1] - piece_off[0])) + 1
    return pieces, piece_off, member_off, members, term_off, term_genes


def _bin_offsets(n_bins, n_groups):
    """bin_off of gat_sample_coverage and the per-bin overlaps: n_groups + 1 entries, the running sum of n_bins"""
    n_bins = np.ascontiguousarray(n_bins, dtype=np.int64)
    assert n_bins.shape == (n_groups,)
    bin_off = np.zeros(n_groups + 1, dtype=np.int64)
    np.cumsum(n_bins, out=bin_off[1:])
    return bin_off


METRICS_WORDS = ("n", "bases", "pairs", "inter", "touched", "outside_pieces", "tail_n", "tail_bases")


def list_metrics(ctx, lists, list_off, n_lists, ws, ws_off, n_groups):
    """the eight sums (METRICS_WORDS; gat_list_metrics) of n_lists x n_groups caller-provided lists -- list l of group g is
    lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]] -- against the n_groups normalized piece lists
    ws[ws_off[g]:ws_off[g + 1]].  Returns int64 [n_lists, n_groups, 8]."""
    lists = np.ascontiguousarray(lists, dtype=SEG)
    ws = np.ascontiguousarray(ws, dtype=SEG)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    ws_off = np.ascontiguousarray(ws_off, dtype=np.int64)
    n_lists, n_groups = int(n_lists), int(n_groups)
    assert len(list_off) == n_lists * n_groups + 1 and len(ws_off) == n_groups + 1
    out = np.zeros((n_lists, n_groups, len(METRICS_WORDS)), dtype=np.int64)
    _check(lib().gat_list_metrics(ctx._h, _p(lists), _p(list_off), n_lists, _p(ws), _p(ws_off), n_groups, _p(out)), ctx._h)
    return out


DISTANCE_WORDS = ("n", "sum", "near", "none")
DISTANCE_SEGMENT_TO_ANNOTATION, DISTANCE_ANNOTATION_TO_SEGMENT = 0, 1


def list_distances(ctx, lists, list_off, n_lists, annos, anno_off, n_tracks, n_groups, direction, max_distance):
    """the four sums (DISTANCE_WORDS; gat_list_distances) of the nearest-interval distances between n_lists x n_groups
    caller-provided lists -- list l of group g is lists[list_off[l * n_groups + g]:list_off[l * n_groups + g + 1]] -- and
    n_tracks x n_groups annotation lists, track t of group g at index t * n_groups + g, summed over the groups.  direction 0:
    from every segment to the track; 1: from every interval of the track to the segment list.  Returns int64
    [n_lists, n_tracks, 4]."""
    lists = np.ascontiguousarray(lists, dtype=SEG)
    annos = np.ascontiguousarray(annos, dtype=SEG)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
    n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
    assert len(list_off) == n_lists * n_groups + 1 and len(anno_off) == n_tracks * n_groups + 1
    out = np.zeros((n_lists, n_tracks, len(DISTANCE_WORDS)), dtype=np.int64)
    _check(lib().gat_list_distances(ctx._h, _p(lists), _p(list_off), n_lists, _p(annos), _p(anno_off), n_tracks, n_groups,
                                    int(direction), int(max_distance), _p(out)), ctx._h)
    return out


SIGNAL_WORDS = ("n", "covered", "hit", "sum")


def list_signal(ctx, lists, list_off, n_lists, pieces, values, piece_off, n_tracks, n_groups):
    """the four sums (SIGNAL_WORDS; gat_list_signal) of n_tracks x n_groups signal tracks -- track t of group g is
    pieces[piece_off[t * n_groups + g]:piece_off[t * n_groups + g + 1]], normalized, with the int32 values beside them -- over
    n_lists x n_groups caller-provided segment lists (the layout of list_distances), summed over the groups.  Returns int64
    [n_lists, n_tracks, 4]."""
    lists = np.ascontiguousarray(lists, dtype=SEG)
    pieces = np.ascontiguousarray(pieces, dtype=SEG)
    values = np.ascontiguousarray(values, dtype=np.int32)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    piece_off = np.ascontiguousarray(piece_off, dtype=np.int64)
    n_lists, n_tracks, n_groups = int(n_lists), int(n_tracks), int(n_groups)
    assert len(list_off) == n_lists * n_groups + 1 and len(piece_off) == n_tracks * n_groups + 1 and len(values) == len(pieces)
    out = np.zeros((n_lists, n_tracks, len(SIGNAL_WORDS)), dtype=np.int64)
    _check(lib().gat_list_signal(ctx._h, _p(lists), _p(list_off), n_lists, _p(pieces), _p(values), _p(piece_off), n_tracks, n_groups,
                                 _p(out)), ctx._h)
    return out


def call_lane_for(n_lanes, asynchronous, timed, serial_state, others_in_flight, lane_busy):
    """The lane (0..n_lanes-1) an enqueued call would take, or -1: the context's stream (gat_call_lane_for: the library's own rule)."""
    busy = np.ascontiguousarray(list(lane_busy) + [0] * 4, dtype=np.int32)
    return int(lib().gat_call_lane_for(int(n_lanes), int(bool(asynchronous)), int(bool(timed)), int(bool(serial_state)),
                                       int(others_in_flight), _p(busy)))


def intersection_sizes(a, a_off, b, b_begin, b_end, n_tracks):
    """(pairs, bases) per track of b: segments and bases of the intersection of the dictionary a (len(a_off) - 1 normalized
    lists) with each of n_tracks dictionaries given as ranges of b (gat_intersection_sizes: the overlap_* columns)."""
    a = np.ascontiguousarray(a, dtype=SEG)
    b = np.ascontiguousarray(b, dtype=SEG)
    a_off = np.ascontiguousarray(a_off, dtype=np.int64)
    b_begin = np.ascontiguousarray(b_begin, dtype=np.int64)
    b_end = np.ascontiguousarray(b_end, dtype=np.int64)
    n_groups = len(a_off) - 1
    assert len(b_begin) == len(b_end) == n_tracks * n_groups
    pairs = np.zeros(n_tracks, dtype=np.int64)
    bases = np.zeros(n_tracks, dtype=np.int64)
    _check(lib().gat_intersection_sizes(_p(a), _p(a_off), n_groups, _p(b), _p(b_begin), _p(b_end), n_tracks, _p(pairs), _p(bases)))
    return pairs, bases


def list_sums(a, begin, end):
    """SegmentList.sum() (a uint32 accumulator, gat/SegmentList.pyx:1607) of every list a[begin[l]:end[l]] (gat_list_sums)"""
    a = np.ascontiguousarray(a, dtype=SEG)
    begin = np.ascontiguousarray(begin, dtype=np.int64)
    end = np.ascontiguousarray(end, dtype=np.int64)
    assert len(begin) == len(end)
    out = np.zeros(len(begin), dtype=np.int64)
    _check(lib().gat_list_sums(_p(a), _p(begin), _p(end), len(begin), _p(out)))
    return out


def isochore_split(arrays, contig_ids, cls_start, cls_end, cls_label, n_classes, truncate):
    """toIsochores of many lists at once (gat_isochore_split, host threads): arrays -- the lists' SEG arrays (contiguous,
    kept alive by the caller), contig_ids[l] -- the contig of list l in the numbering of the class segments' coordinates.
    Returns (out, out_off): list (l, k) = out[out_off[l * n_classes + k]:out_off[l * n_classes + k + 1]]; None if a list is
    not normalized (the caller's list-by-list form raises what the reference raises)."""
    n = len(arrays)
    # (the address of a list's data: the buffer protocol is the cheapest way to it -- 1 us; __array_interface__ of a structured
    #  array builds its descriptor every time, 7 us; an empty list has no buffer to speak of and is never read)
    addr, from_buffer = C.addressof, C.c_char.from_buffer
    ptr = np.fromiter((addr(from_buffer(a)) if len(a) and a.flags["WRITEABLE"] else a.ctypes.data for a in arrays),
                      dtype=np.uint64, count=n)
    lens = np.fromiter((len(a) for a in arrays), dtype=np.int64, count=n)
    cid = np.ascontiguousarray(contig_ids, dtype=np.int64)
    cls_start = np.ascontiguousarray(cls_start, dtype=np.int64)
    cls_end = np.ascontiguousarray(cls_end, dtype=np.int64)
    cls_label = np.ascontiguousarray(cls_label, dtype=np.int64)
    off = np.zeros(n * n_classes + 1, dtype=np.int64)
    total = C.c_int64(0)
    args = (_p(ptr), _p(lens), _p(cid), n, _p(cls_start), _p(cls_end), _p(cls_label), len(cls_start), int(n_classes), 1 if truncate else 0)
    rc = lib().gat_isochore_split(*args, None, _p(off), C.byref(total))
    if rc == 1:
        return None
    _check(rc)
    out = np.empty(max(1, total.value), dtype=SEG)
    _check(lib().gat_isochore_split(*args, _p(out), _p(off), C.byref(total)))
    return out[:total.value], off


COMM_ID_BYTES = 128


def comm_unique_id():
    """128 bytes that rank 0 hands to the other ranks (ncclGetUniqueId through the C ABI)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().gat_comm_unique_id(buf))
    return buf.raw


class Comm(object):
    """RCCL communicator of the C ABI (gat_comm): the all-gather of the per-rank count blocks without torch."""

    def __init__(self, ctx, n_ranks, rank, unique_id):
        self.ctx, self.n_ranks, self.rank = ctx, n_ranks, rank
        self._h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _check(lib().gat_comm_create(ctx._h, C.byref(self._h), int(n_ranks), int(rank), buf), ctx._h)

    def allgather_counts(self, send_dev_ptr, recv_dev_ptr, n_slots):
        _check(lib().gat_allgather_counts(self.ctx._h, self._h, C.c_void_p(send_dev_ptr), C.c_void_p(recv_dev_ptr), int(n_slots)),
               self.ctx._h)

    def close(self):
        if self._h:
            lib().gat_comm_destroy(self._h)
            self._h = C.c_void_p()


class Annotations(object):
    """the annotation side of a problem as a device-resident object of its own (gat_annotations): made once per run(),
    shared by the problems of every segment track whose contigs are `flat`'s (same names, same order)."""

    def __init__(self, ctx, flat, mean_segment_length=0.0, asynchronous=False, nucleotide_only=False):
        """asynchronous: the tables are built by a thread of the library while the caller goes on (GAT_ANNOTATIONS_ASYNC);
        the arrays handed over stay referenced by this object.  nucleotide_only: only the nucleotide counters will be asked
        for (GAT_ANNOTATIONS_NUCLEOTIDE_ONLY: where the merged index is built the per-track tables are left out)."""
        self.ctx = ctx
        keep = self._keep = {}

        def arr(name, dtype):
            keep[name] = np.ascontiguousarray(flat[name], dtype=dtype)
            return _p(keep[name])

        d = AnnotationsDesc()
        d.n_tracks, d.n_contigs, d.merge_contigs = int(flat["n_tracks"]), int(flat["n_contigs"]), int(flat["merge_contigs"])
        d.annos = arr("annos", SEG)
        d.anno_off = arr("anno_off", np.int64)
        if flat.get("anno_group") is not None:
            d.n_anno_lists = len(flat["anno_group"])
            d.anno_group = arr("anno_group", np.int32)
            d.anno_end = arr("anno_end", np.int64)
            assert len(keep["anno_off"]) == len(keep["anno_end"]) == d.n_anno_lists
        else:
            assert len(keep["anno_off"]) == d.n_tracks * d.n_contigs + 1
        d.mean_segment_length = float(mean_segment_length)
        d.flags = (1 if asynchronous else 0) | (2 if nucleotide_only else 0)
        self.n_tracks, self.n_contigs, self.merge_contigs = d.n_tracks, d.n_contigs, d.merge_contigs
        self._h = C.c_void_p()
        _check(lib().gat_annotations_create(ctx._h, C.byref(d), C.byref(self._h)), ctx._h)

    def wait(self):
        """an asynchronous build has finished (raises its error, if any)"""
        _check(lib().gat_annotations_wait(self.ctx._h, self._h), self.ctx._h)

    def close(self):
        if self._h:
            if getattr(self.ctx, "_h", None):
                lib().gat_annotations_wait(self.ctx._h, self._h)     # (a build still running has the arrays below in use)
            lib().gat_annotations_destroy(self._h)
            self._h = C.c_void_p()
        self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Problem(object):
    """device-resident inputs of one segment track (gat_problem).

    `flat` is a mapping with the fields of gat_problem_desc (numpy arrays / ints); annotations: an Annotations object made
    for the same tracks and contigs (flat's annotation lists are then not looked at and may be missing)."""

    def __init__(self, ctx, flat, annotations=None):
        self.ctx = ctx
        keep = {}

        def arr(name, dtype):
            keep[name] = np.ascontiguousarray(flat[name], dtype=dtype)
            return _p(keep[name])

        d = ProblemDesc()
        d.n_units = int(flat["n_units"])
        d.segs = arr("segs", SEG)
        d.seg_off = arr("seg_off", np.int64)
        d.ws = arr("ws", SEG)
        d.ws_off = arr("ws_off", np.int64)
        d.unit_contig = arr("unit_contig", np.int32)
        d.n_contigs = int(flat["n_contigs"])
        d.merge_contigs = int(flat["merge_contigs"])
        d.n_tracks = int(flat["n_tracks"])
        if annotations is None:
            d.annos = arr("annos", SEG)
            d.anno_off = arr("anno_off", np.int64)
        else:
            d.annotations = annotations._h
        d.cws_nseg = arr("cws_nseg", np.int64)
        d.bucket_size = int(flat.get("bucket_size", 0))
        d.nbuckets = int(flat.get("nbuckets", 100000))
        d.sampler = int(flat.get("sampler", 0))
        d.shift_radius = float(flat.get("shift_radius", 2.0))
        d.shift_extension = int(flat.get("shift_extension", 0))
        d.brute_ntries_inner = int(flat.get("brute_ntries_inner", 0))
        d.brute_ntries_outer = int(flat.get("brute_ntries_outer", 0))
        assert len(keep["seg_off"]) == d.n_units + 1 and len(keep["ws_off"]) == d.n_units + 1
        assert len(keep["cws_nseg"]) == d.n_contigs
        if annotations is not None:
            pass
        elif flat.get("anno_group") is not None:
            # the annotation lists as the host holds them (one per track and key), grouped into contigs by the library
            d.n_anno_lists = len(flat["anno_group"])
            d.anno_group = arr("anno_group", np.int32)
            d.anno_end = arr("anno_end", np.int64)
            assert len(keep["anno_off"]) == len(keep["anno_end"]) == d.n_anno_lists
        else:
            assert len(keep["anno_off"]) == d.n_tracks * d.n_contigs + 1
        self.n_units, self.n_contigs, self.n_tracks = d.n_units, d.n_contigs, d.n_tracks
        self._h = C.c_void_p()
        _check(lib().gat_problem_create(ctx._h, C.byref(d), C.byref(self._h)), ctx._h)
        self.last_stats = None

    def close(self):
        if self._h:
            lib().gat_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        v = [C.c_int64() for _ in range(5)]
        _check(lib().gat_problem_info(self._h, *[C.byref(x) for x in v]))
        return dict(n_units=v[0].value, n_contigs=v[1].value, n_tracks=v[2].value,
                    slab_segments_per_sample=v[3].value, algorithmic_bytes_per_sample=v[4].value)

    def rows_per_sample(self):
        """raw MT19937 outputs generated ahead per sample, over all units (the rows of k_rng)"""
        return int(lib().gat_problem_rng_rows(self._h))

    def sample_and_count_device(self, counters, seed, sample_begin, sample_end, counts_dev_ptr):
        """the batch seam, results left on the device ([counter][track][sample] 8-byte slots)."""
        ids = np.array([COUNTER_IDS[c] for c in counters], dtype=np.int32)
        st = Stats()
        rc = lib().gat_sample_and_count(self.ctx._h, self._h, _p(ids), len(ids), int(seed) & 0xFFFFFFFF,
                                        int(sample_begin), int(sample_end), C.c_void_p(counts_dev_ptr), C.byref(st))
        self.last_stats = st.asdict()           # (of a failed call too: SamplerBruteForce's n_unconverged)
        _check(rc, self.ctx._h)
        return self.last_stats

    def enqueue(self, counters, seed, sample_begin, sample_end, counts_dev_ptr):
        """first half of the batch seam (gat_sample_and_count_enqueue): the call's batches are put on the context's stream
        and the host goes on; counts_dev_ptr must stay valid until wait()."""
        ids = np.array([COUNTER_IDS[c] for c in counters], dtype=np.int32)
        _check(lib().gat_sample_and_count_enqueue(self.ctx._h, self._h, _p(ids), len(ids), int(seed) & 0xFFFFFFFF,
                                                  int(sample_begin), int(sample_end), C.c_void_p(counts_dev_ptr)), self.ctx._h)

    def wait(self):
        """second half (gat_wait): blocks until the call has completed, raises what sample_and_count_device would have"""
        st = Stats()
        rc = lib().gat_wait(self.ctx._h, self._h, C.byref(st))
        self.last_stats = st.asdict()
        _check(rc, self.ctx._h)
        return self.last_stats

    def sample_and_count(self, counters, seed, sample_begin, sample_end):
        """returns a list (per counter) of [n_tracks, n_samples] arrays (int64 / float64 for density)."""
        ns = sample_end - sample_begin
        nslots = max(1, len(counters) * self.n_tracks * ns)
        dev = self.ctx.alloc(nslots * 8)
        try:
            self.sample_and_count_device(counters, seed, sample_begin, sample_end, dev)
            host = np.empty((len(counters), self.n_tracks, ns), dtype=np.int64)
            if host.size:
                self.ctx.d2h(host, dev)
        finally:
            self.ctx.free(dev)
        return [host[k].view(np.float64) if c == "nucleotide-density" else host[k] for k, c in enumerate(counters)]

    def sample_and_count_serial(self, counters, mt_state, n_samples):
        """samples 0 .. n_samples-1 drawn from ONE MT19937 stream in the reference's order (an unpatched gat-run.py
        --random-seed): mt_state (mt19937_seed(seed), or what an earlier call left) is advanced in place.  Returns the
        count matrices like sample_and_count."""
        assert mt_state.dtype == np.uint32 and mt_state.size == MT_STATE_WORDS and mt_state.flags["C_CONTIGUOUS"]
        ids = np.array([COUNTER_IDS[c] for c in counters], dtype=np.int32)
        ns = int(n_samples)
        dev = self.ctx.alloc(max(1, len(counters) * self.n_tracks * ns) * 8)
        st = Stats()
        try:
            _check(lib().gat_sample_and_count_serial(self.ctx._h, self._h, _p(ids), len(ids), _p(mt_state), ns,
                                                     C.c_void_p(dev), C.byref(st)), self.ctx._h)
            host = np.zeros((len(counters), self.n_tracks, ns), dtype=np.int64)
            if host.size:
                self.ctx.d2h(host, dev)
        finally:
            self.ctx.free(dev)
        self.last_stats = st.asdict()
        return [host[k].view(np.float64).copy() if c == "nucleotide-density" else host[k].copy()
                for k, c in enumerate(counters)]

    def sample(self, seed, sample_begin, sample_end, unit_level=False):
        """sampled contig-level segment lists: (segments SEG array, offsets[(n_samples*n_contigs)+1]); with
        unit_level the lists of every (sample, unit) as the sampler returned them (offsets per n_units)."""
        ns = sample_end - sample_begin
        off = np.zeros(ns * (self.n_units if unit_level else self.n_contigs) + 1, dtype=np.int64)
        cap = max(1024, self.info()["slab_segments_per_sample"] * ns // 2)
        st = Stats()
        fn = lib().gat_sample_units if unit_level else lib().gat_sample
        while True:
            out = np.empty(cap, dtype=SEG)
            rc = fn(self.ctx._h, self._h, int(seed) & 0xFFFFFFFF, int(sample_begin), int(sample_end),
                    _p(out), cap, _p(off), C.byref(st))
            if rc == -3 and off[-1] > cap:
                cap = int(off[-1])
                continue
            self.last_stats = st.asdict()
            _check(rc, self.ctx._h)
            break
        return out[: off[-1]].copy(), off

    def sample_coverage(self, seed, sample_begin, sample_end, bin_size, n_bins, want_starts_ends=True):
        """per-bin coverage of the sampled contig-level lists, summed over the samples (gat_sample_coverage): n_bins[c] bins
        of bin_size bases for contig c.  Returns (bases, starts, ends, outside, bin_off): int64 arrays, contig c's bins at
        [bin_off[c], bin_off[c + 1]); starts and ends are None unless wanted; outside[c]: sampled bases beyond the last bin."""
        n_bins = np.ascontiguousarray(n_bins, dtype=np.int64)
        assert n_bins.shape == (self.n_contigs,)
        bin_off = np.zeros(self.n_contigs + 1, dtype=np.int64)
        np.cumsum(n_bins, out=bin_off[1:])
        total = max(0, int(bin_off[-1]))
        bases = np.zeros(total, dtype=np.int64)
        starts = np.zeros(total, dtype=np.int64) if want_starts_ends else None
        ends = np.zeros(total, dtype=np.int64) if want_starts_ends else None
        outside = np.zeros(self.n_contigs, dtype=np.int64)
        st = Stats()
        rc = lib().gat_sample_coverage(self.ctx._h, self._h, int(seed) & 0xFFFFFFFF, int(sample_begin), int(sample_end),
                                       int(bin_size), _p(bin_off), _p(bases), _p(starts), _p(ends), _p(outside), C.byref(st))
        self.last_stats = st.asdict()
        _check(rc, self.ctx._h)
        return bases, starts, ends, outside, bin_off

    def sample_metrics(self, seed, sample_begin, sample_end, ws, ws_off):
        """the eight sums (METRICS_WORDS; gat_sample_metrics) of every sampled contig-level list of [sample_begin, sample_end)
        against the pieces ws[ws_off[c]:ws_off[c + 1]] of contig c, in the problem's contig order.  Returns int64
        [samples, n_contigs, 8]."""
        ws = np.ascontiguousarray(ws, dtype=SEG)
        ws_off = np.ascontiguousarray(ws_off, dtype=np.int64)
        assert ws_off.shape == (self.n_contigs + 1,)
        out = np.zeros((max(0, int(sample_end) - int(sample_begin)), self.n_contigs, len(METRICS_WORDS)), dtype=np.int64)
        st = Stats()
        rc = lib().gat_sample_metrics(self.ctx._h, self._h, int(seed) & 0xFFFFFFFF, int(sample_begin), int(sample_end),
                                      _p(ws), _p(ws_off), _p(out), C.byref(st))
        self.last_stats = st.asdict()
        _check(rc, self.ctx._h)
        return out

    def sample_distances(self, seed, sample_begin, sample_end, annos, anno_off, n_tracks, direction, max_distance):
        """the four sums (DISTANCE_WORDS; gat_sample_distances) of the nearest-interval distances between every sampled
        contig-level list of [sample_begin, sample_end) and n_tracks annotation tracks -- track t of contig c is
        annos[anno_off[t * n_contigs + c]:anno_off[t * n_contigs + c + 1]], contigs in the problem's order -- summed over the
        contigs.  Returns int64 [samples, n_tracks, 4]."""
        annos = np.ascontiguousarray(annos, dtype=SEG)
        anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
        n_tracks = int(n_tracks)
        assert anno_off.shape == (n_tracks * self.n_contigs + 1,)
        out = np.zeros((max(0, int(sample_end) - int(sample_begin)), n_tracks, len(DISTANCE_WORDS)), dtype=np.int64)
        st = Stats()
        rc = lib().gat_sample_distances(self.ctx._h, self._h, int(seed) & 0xFFFFFFFF, int(sample_begin), int(sample_end),
                                        _p(annos), _p(anno_off), n_tracks, int(direction), int(max_distance), _p(out), C.byref(st))
        self.last_stats = st.asdict()
        _check(rc, self.ctx._h)
        return out

    def sample_signal(self, seed, sample_begin, sample_end, pieces, values, piece_off, n_tracks):
        """the four sums (SIGNAL_WORDS; gat_sample_signal) of n_tracks signal tracks -- track t of contig c is
        pieces[piece_off[t * n_contigs + c]:piece_off[t * n_contigs + c + 1]] with the int32 values beside them, contigs in the
        problem's order -- over every sampled contig-level list of [sample_begin, sample_end), summed over the contigs.
        Returns int64 [samples, n_tracks, 4]."""
        pieces = np.ascontiguousarray(pieces, dtype=SEG)
        values = np.ascontiguousarray(values, dtype=np.int32)
        piece_off = np.ascontiguousarray(piece_off, dtype=np.int64)
        n_tracks = int(n_tracks)
        assert piece_off.shape == (n_tracks * self.n_contigs + 1,) and len(values) == len(pieces)
        out = np.zeros((max(0, int(sample_end) - int(sample_begin)), n_tracks, len(SIGNAL_WORDS)), dtype=np.int64)
        st = Stats()
        rc = lib().gat_sample_signal(self.ctx._h, self._h, int(seed) & 0xFFFFFFFF, int(sample_begin), int(sample_end),
                                     _p(pieces), _p(values), _p(piece_off), n_tracks, _p(out), C.byref(st))
        self.last_stats = st.asdict()
        _check(rc, self.ctx._h)
        return out

    def _sample_null_words(self, call, seed, sample_begin, sample_end, args, obs, cells):
        """the tail of the three calls below: call(ctx, problem, seed, the range, *args, obs, out, stats) fills NULL_WORDS per
        cell of an int64 array of shape `cells`, which is returned"""
        out = np.zeros(tuple(cells) + (len(NULL_WORDS),), dtype=np.int64)
        st = Stats()
        rc = call(self.ctx._h, self._h, int(seed) & 0xFFFFFFFF, int(sample_begin), int(sample_end), *args, _p(obs), _p(out), C.byref(st))
        self.last_stats = st.asdict()
        _check(rc, self.ctx._h)
        return out

    def sample_bin_enrichment(self, seed, sample_begin, sample_end, annos, anno_off, n_tracks, bin_size, n_bins, obs):
        """per (track, bin) the five sums (LOCAL_WORDS; gat_sample_bin_enrichment) over the sampled contig-level lists of
        [sample_begin, sample_end) of v = the bases a list shares with the track inside the bin, against obs[track, bin] --
        track t of contig c is annos[anno_off[t * n_contigs + c]:anno_off[t * n_contigs + c + 1]], n_bins[c] bins of bin_size
        bases for contig c, contigs in the problem's order.  Returns (words, bin_off): int64 [n_tracks, total_bins, 5]."""
        annos = np.ascontiguousarray(annos, dtype=SEG)
        anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
        n_tracks = int(n_tracks)
        assert anno_off.shape == (n_tracks * self.n_contigs + 1,)
        bin_off = _bin_offsets(n_bins, self.n_contigs)
        total = max(0, int(bin_off[-1]))
        obs = np.ascontiguousarray(obs, dtype=np.int64)
        assert obs.shape == (n_tracks, total)
        return self._sample_null_words(lib().gat_sample_bin_enrichment, seed, sample_begin, sample_end,
                                       (_p(annos), _p(anno_off), n_tracks, int(bin_size), _p(bin_off)), obs, (n_tracks, total)), bin_off

    def sample_pair_enrichment(self, seed, sample_begin, sample_end, annos, anno_off, n_tracks, obs):
        """per pair (i, j), i <= j, of n_tracks tracks the five sums (PAIR_WORDS; gat_sample_pair_enrichment) over the sampled
        contig-level lists of [sample_begin, sample_end) of c = the segments of a list that hit track i and track j, against
        obs[pair] -- track t of contig c is annos[anno_off[t * n_contigs + c]:anno_off[t * n_contigs + c + 1]], contigs in
        the problem's order.  Returns int64 [P, 5]."""
        annos = np.ascontiguousarray(annos, dtype=SEG)
        anno_off = np.ascontiguousarray(anno_off, dtype=np.int64)
        n_tracks = int(n_tracks)
        assert anno_off.shape == (max(0, n_tracks) * self.n_contigs + 1,)
        obs = np.ascontiguousarray(obs, dtype=np.int64)
        assert not 0 <= n_tracks <= PAIR_MAX_TRACKS or obs.shape == (pair_count(n_tracks),)
        return self._sample_null_words(lib().gat_sample_pair_enrichment, seed, sample_begin, sample_end,
                                       (_p(annos), _p(anno_off), n_tracks), obs, (pair_count(n_tracks),))

    def sample_geneset_enrichment(self, seed, sample_begin, sample_end, pieces, piece_off, member_off, members, n_genes, term_off,
                                  term_genes, n_terms, obs):
        """per term the five sums (GENESET_WORDS; gat_sample_geneset_enrichment) over the sampled contig-level lists of
        [sample_begin, sample_end) of c = the genes of the term hit by any segment of a list, against obs[term] -- the genes'
        pieces of contig c are pieces[piece_off[c]:piece_off[c + 1]], contigs in the problem's order; the other arguments as
        in Context.list_geneset_hits.  Returns int64 [n_terms, 5]."""
        n_genes, n_terms = int(n_genes), int(n_terms)
        g = _geneset_arrays(pieces, piece_off, member_off, members, term_off, term_genes, n_terms, self.n_contigs)
        obs = np.ascontiguousarray(obs, dtype=np.int64)
        assert obs.shape == (max(0, n_terms),)
        return self._sample_null_words(lib().gat_sample_geneset_enrichment, seed, sample_begin, sample_end,
                                       (_p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), n_genes, _p(g[4]), _p(g[5]), n_terms), obs, (max(0, n_terms),))

    def sample_profile_enrichment(self, seed, sample_begin, sample_end, anchor_pos, anchor_minus, anchor_off, n_tracks, bin_size,
                                  half_bins, mode, obs):
        """per (track, offset bin) the five sums (PROFILE_WORDS; gat_sample_profile_enrichment) over the sampled contig-level
        lists of [sample_begin, sample_end) of v = the bases (mode PROFILE_BASES) or segment midpoints (PROFILE_MIDPOINTS) of
        a list in the bin around the track's anchors, against obs[track, bin] -- the anchors as in Context.list_profile, the
        groups the problem's contigs in the problem's order.  Returns int64 [n_tracks, 2 * half_bins, 5]."""
        n_tracks = int(n_tracks)
        pos, minus, anchor_off = _profile_arrays(anchor_pos, anchor_minus, anchor_off, n_tracks, self.n_contigs)
        cells = (max(0, n_tracks), profile_bins(half_bins))
        obs = np.ascontiguousarray(obs, dtype=np.int64)
        assert obs.shape == cells
        return self._sample_null_words(lib().gat_sample_profile_enrichment, seed, sample_begin, sample_end,
                                       (_p(pos), _p(minus), _p(anchor_off), n_tracks, int(bin_size), int(half_bins), int(mode)), obs, cells)

    def sample_reldist_enrichment(self, seed, sample_begin, sample_end, point_pos, point_off, n_tracks, n_bins, obs):
        """per (track, value) the five sums (RELDIST_WORDS; gat_sample_reldist_enrichment) over the sampled contig-level
        lists of [sample_begin, sample_end) of the list's relative distance values -- the bins, area, inside, outside -- against
        obs[track, value]; the points as in Context.list_reldist, the groups the problem's contigs in the problem's order.
        Returns int64 [n_tracks, n_bins + RELDIST_EXTRA, 5]."""
        n_tracks = int(n_tracks)
        pos, point_off = _reldist_arrays(point_pos, point_off, n_tracks, self.n_contigs)
        cells = (max(0, n_tracks), reldist_values(n_bins))
        obs = np.ascontiguousarray(obs, dtype=np.int64)
        assert obs.shape == cells
        return self._sample_null_words(lib().gat_sample_reldist_enrichment, seed, sample_begin, sample_end,
                                       (_p(pos), _p(point_off), n_tracks, int(n_bins)), obs, cells)

    def sample_metagene_enrichment(self, seed, sample_begin, sample_end, feat_start, feat_end, feat_minus, feat_off, n_tracks,
                                   body_bins, flank_bins, flank_bin_size, mode, obs):
        """per (track, bin) the five sums (METAGENE_WORDS; gat_sample_metagene_enrichment) over the sampled contig-level lists
        of [sample_begin, sample_end) of v = the bases (mode METAGENE_BASES) or segment midpoints (METAGENE_MIDPOINTS) of a
        list in the bin along the track's scaled features and their flanks, against obs[track, bin] -- the features as in
        Context.list_metagene, the groups the problem's contigs in the problem's order.  Returns int64
        [n_tracks, 2 * flank_bins + body_bins, 5]."""
        n_tracks = int(n_tracks)
        fs, fe, minus, feat_off = _metagene_arrays(feat_start, feat_end, feat_minus, feat_off, n_tracks, self.n_contigs)
        cells = (max(0, n_tracks), metagene_bins(body_bins, flank_bins))
        obs = np.ascontiguousarray(obs, dtype=np.int64)
        assert obs.shape == cells
        return self._sample_null_words(lib().gat_sample_metagene_enrichment, seed, sample_begin, sample_end,
                                       (_p(fs), _p(fe), _p(minus), _p(feat_off), n_tracks, int(body_bins), int(flank_bins),
                                        int(flank_bin_size), int(mode)), obs, cells)
