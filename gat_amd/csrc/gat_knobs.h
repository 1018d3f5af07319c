// gat_knobs.h -- the run-time tuning / testing knobs (GAT_*) the library reads, declared ONCE: field,
// name, default.  read_knobs resolves all of them under one lock -- a context's own value (gat_ctx_set_option), else the
// process's environment as it was when the library first looked -- into a plain struct returned by value; nothing points into
// a context's option map.  A snapshot is taken at three moments and only there: when a problem is created, when annotation
// tables are created (kept in the gat_annotations object: the build, on whatever thread, reads that one), and at the top of
// a call (kept with the call in flight: every batch of it sees the same values).  A set_option acts on what starts after it.
// A value "" is "not set".  FLAG: set at all.  INT / REAL: atoll / atof of the value, `x_set` beside it where presence
// matters apart from the value.  TEXT: the string, empty when not set.
#pragma once
#include <cstdint>
#include <string>

struct gat_ctx;

#define GAT_KNOBS(FLAG, INT, REAL, TEXT)                                                                                     \
  /* the process's (read_knobs(nullptr) / process_knobs(): no context where they act) */                                     \
  REAL(pool_bytes, "GAT_POOL_BYTES", 96.0 * 1024 * 1024 * 1024)                                                              \
  INT(host_threads, "GAT_HOST_THREADS", 0) /* default: min(16, cores) */                                                     \
  INT(host_pool, "GAT_HOST_POOL", 1)                                                                                         \
  FLAG(time_create, "GAT_TIME_CREATE")                                                                                       \
  TEXT(rccl_lib, "GAT_RCCL_LIB")                                                                                             \
  /* problem creation */                                                                                                     \
  FLAG(place_no_grid, "GAT_PLACE_NO_GRID")                                                                                   \
  FLAG(tail_no_long_ws, "GAT_TAIL_NO_LONG_WS")                                                                               \
  FLAG(no_split, "GAT_NO_SPLIT")                                                                                             \
  TEXT(sampler_mode, "GAT_SAMPLER_MODE")                                                                                     \
  REAL(rng_slack, "GAT_RNG_SLACK", 1.0)                                                                                      \
  REAL(rng_sigma_min, "GAT_RNG_SIGMA_MIN", 3.5)                                                                              \
  REAL(rng_sigma_max, "GAT_RNG_SIGMA_MAX", 7.5)                                                                              \
  REAL(rng_tail_rows, "GAT_RNG_TAIL_ROWS", 0.0) /* default: by the unit */                                                   \
  INT(grid_cell_segs, "GAT_GRID_CELL_SEGS", 2)                                                                               \
  /* problem creation and the call (a layout made again; the count route) */                                                 \
  FLAG(test_small_caps, "GAT_TEST_SMALL_CAPS")                                                                               \
  INT(size_classes, "GAT_SIZE_CLASSES", 6)                                                                                   \
  FLAG(count_via_contigs, "GAT_COUNT_VIA_CONTIGS")                                                                           \
  /* annotation tables */                                                                                                    \
  INT(merged_min_tracks, "GAT_MERGED_MIN_TRACKS", 4)                                                                         \
  INT(merged_bound, "GAT_MERGED_BOUND", 2)                                                                                   \
  INT(merged_block, "GAT_MERGED_BLOCK", 0) /* default: by the expected length of a scan */                                   \
  INT(grid_factor, "GAT_GRID_FACTOR", 2)                                                                                     \
  INT(annotations_sync, "GAT_ANNOTATIONS_SYNC", 0)                                                                           \
  /* annotation tables and the call */                                                                                       \
  INT(count_lds_entries, "GAT_COUNT_LDS_ENTRIES", 1024)                                                                      \
  FLAG(count_no_merged, "GAT_COUNT_NO_MERGED")                                                                               \
  /* the call */                                                                                                             \
  REAL(slab_bytes, "GAT_SLAB_BYTES", 72.0 * 1024 * 1024 * 1024)                                                              \
  INT(call_lanes, "GAT_CALL_LANES", 2)                                                                                       \
  FLAG(kernel_times, "GAT_KERNEL_TIMES")                                                                                     \
  TEXT(diag_out, "GAT_DIAG_OUT")                                                                                             \
  FLAG(test_huge, "GAT_TEST_HUGE")                                                                                           \
  FLAG(no_merge_big, "GAT_NO_MERGE_BIG")                                                                                     \
  FLAG(no_tail_big, "GAT_NO_TAIL_BIG")                                                                                       \
  FLAG(no_resume_big, "GAT_NO_RESUME_BIG")                                                                                   \
  FLAG(no_long_queue, "GAT_NO_LONG_QUEUE")                                                                                   \
  FLAG(lperm_simple, "GAT_LPERM_SIMPLE")                                                                                     \
  FLAG(exp_lperm_no_normalize, "GAT_EXP_LPERM_NO_NORMALIZE")                                                                 \
  FLAG(place_no_cm, "GAT_PLACE_NO_CM")                                                                                       \
  FLAG(place_no_wide, "GAT_PLACE_NO_WIDE")                                                                                   \
  FLAG(place_wide, "GAT_PLACE_WIDE")                                                                                         \
  INT(place_scan_tiles, "GAT_PLACE_SCAN_TILES", 768)                                                                         \
  FLAG(place_scan_seq, "GAT_PLACE_SCAN_SEQ")                                                                                 \
  FLAG(place_no_pipe, "GAT_PLACE_NO_PIPE")                                                                                   \
  FLAG(merge_old, "GAT_MERGE_OLD")                                                                                           \
  INT(merge_buckets, "GAT_MERGE_BUCKETS", 8192)                                                                              \
  FLAG(resume_compact, "GAT_RESUME_COMPACT")                                                                                 \
  FLAG(resume_insert, "GAT_RESUME_INSERT")                                                                                   \
  INT(tb_no_bridge, "GAT_TB_NO_BRIDGE", 0)                                                                                   \
  FLAG(tb_no_log_map, "GAT_TB_NO_LOG_MAP")                                                                                   \
  FLAG(consolidate_slab_lds, "GAT_CONSOLIDATE_SLAB_LDS")                                                                     \
  FLAG(contig_final_lists, "GAT_CONTIG_FINAL_LISTS")                                                                         \
  FLAG(no_wpe5, "GAT_NO_WPE5")                                                                                               \
  FLAG(count_final_lists, "GAT_COUNT_FINAL_LISTS")                                                                           \
  FLAG(count_no_swap, "GAT_COUNT_NO_SWAP")                                                                                   \
  INT(count_samples_per_block, "GAT_COUNT_SAMPLES_PER_BLOCK", 32)                                                            \
  INT(count_tracks_per_block, "GAT_COUNT_TRACKS_PER_BLOCK", 16)                                                              \
  INT(count_staged, "GAT_COUNT_STAGED", 1)                                                                                   \
  INT(merged_samples_per_block, "GAT_MERGED_SAMPLES_PER_BLOCK", 4)                                                           \
  FLAG(count_lists_merged, "GAT_COUNT_LISTS_MERGED")                                                                         \
  INT(null_fold_parts, "GAT_NULL_FOLD_PARTS", 0) /* gat_null_fold: workgroups a row is cut over, 1 .. 1024; default: by the launch */ \
  REAL(compare_scratch_mb, "GAT_COMPARE_SCRATCH_MB", 1024.0) /* gat_compare_stats: megabytes of transformed rows per batch */ \
  INT(coverage_window_bins, "GAT_COVERAGE_WINDOW_BINS", 1920) /* gat_sample_coverage: bins of a workgroup's LDS window */      \
  INT(coverage_samples_per_block, "GAT_COVERAGE_SAMPLES_PER_BLOCK", 0) /* ... its chunk of samples; default: by the launch */ \
  INT(metrics_lds_pieces, "GAT_METRICS_LDS_PIECES", 2048) /* gat_*_metrics: pieces of a group k_metrics' searches find in LDS */ \
  INT(distance_lds_pieces, "GAT_DISTANCE_LDS_PIECES", 2048) /* gat_*_distances: intervals of a list k_distance's search finds in LDS */ \
  INT(signal_lds_pieces, "GAT_SIGNAL_LDS_PIECES", 2048) /* gat_*_signal: piece ends of a (track, group) k_signal's searches find in LDS */ \
  INT(minp_lds_samples, "GAT_MINP_LDS_SAMPLES", 4096) /* gat_minp_counts: samples per row up to which k_minp_rank sorts in LDS */   \
  REAL(minp_scratch_mb, "GAT_MINP_SCRATCH_MB", 1024.0) /* ... megabytes of K (4 bytes a sample) per batch of rows */                \
  FLAG(minp_all_passes, "GAT_MINP_ALL_PASSES") /* ... the sort runs all 16 digit passes (measuring what the skip is worth) */      \
  INT(efdr_lds_thresholds, "GAT_EFDR_LDS_THRESHOLDS", 0) /* gat_efdr_counts: thresholds per pass of k_efdr; default: what a workgroup's LDS holds */ \
  INT(local_window_bins, "GAT_LOCAL_WINDOW_BINS", 256) /* gat_*_bin_*: bins of a workgroup's LDS window in k_local */          \
  INT(local_samples_per_block, "GAT_LOCAL_SAMPLES_PER_BLOCK", 0) /* ... its run of lists; default: by the launch */            \
  INT(local_lds_pieces, "GAT_LOCAL_LDS_PIECES", 256) /* ... annotation intervals of a window its search finds in LDS */       \
  INT(pairs_lds_pieces, "GAT_PAIRS_LDS_PIECES", 32) /* gat_*_pair_*: intervals of a (track, group) k_pairs' search finds in LDS; 0: none */ \
  INT(pairs_samples_per_block, "GAT_PAIRS_SAMPLES_PER_BLOCK", 0) /* ... its run of lists; default: by the launch */            \
  INT(geneset_lds_pieces, "GAT_GENESET_LDS_PIECES", 1024) /* gat_*_geneset_*: piece ends of a group k_geneset_hits' searches find in LDS; 0: none */ \
  INT(geneset_samples_per_block, "GAT_GENESET_SAMPLES_PER_BLOCK", 0) /* ... the run of lists of both kernels; default: by the launch */ \
  INT(geneset_term_tile, "GAT_GENESET_TERM_TILE", 256) /* ... terms a workgroup of k_geneset_terms owns, 1 .. 256 */           \
  INT(profile_lds_anchors, "GAT_PROFILE_LDS_ANCHORS", 1024) /* gat_*_profile*: anchor positions of a (track, group) k_profile's search finds in LDS; 0: none */ \
  INT(profile_samples_per_block, "GAT_PROFILE_SAMPLES_PER_BLOCK", 0) /* ... its run of lists; default: by the launch */ \
  INT(reldist_lds_points, "GAT_RELDIST_LDS_POINTS", 1024) /* gat_*_reldist*: positions of a (track, group) k_reldist's search finds in LDS; 0: none */ \
  INT(reldist_samples_per_block, "GAT_RELDIST_SAMPLES_PER_BLOCK", 0) /* ... its run of lists; default: by the launch */ \
  INT(metagene_lds_features, "GAT_METAGENE_LDS_FEATURES", 1024) /* gat_*_metagene*: prefix maxima of the ends of a (track, group) k_metagene's search finds in LDS; 0: none */ \
  INT(metagene_samples_per_block, "GAT_METAGENE_SAMPLES_PER_BLOCK", 0) /* ... its run of lists; default: by the launch */

struct Knobs {
#define GAT_KNOB_FLAG(field, name) bool field = false;
#define GAT_KNOB_INT(field, name, dflt) int64_t field = dflt; bool field##_set = false;
#define GAT_KNOB_REAL(field, name, dflt) double field = dflt; bool field##_set = false;
#define GAT_KNOB_TEXT(field, name) std::string field;
  GAT_KNOBS(GAT_KNOB_FLAG, GAT_KNOB_INT, GAT_KNOB_REAL, GAT_KNOB_TEXT)
#undef GAT_KNOB_FLAG
#undef GAT_KNOB_INT
#undef GAT_KNOB_REAL
#undef GAT_KNOB_TEXT
};

Knobs read_knobs(const gat_ctx* ctx);     // gat_prep.hip; nullptr: the process's values
const Knobs& process_knobs();             // read_knobs(nullptr), made once (the environment's snapshot does not change)
