/*
 * gat_mi355.h -- C ABI of libgat_mi355.so: the MI355X (gfx950) implementation of GAT's
 * Monte-Carlo sampling + overlap-counting hot path.
 *
 * The reference (AndreasHeger/gat 1.3.6) has no FFI; its seams for this path are Python-level
 * calls into Cython cdef classes.  Each entry point below names the reference
 * interface it replaces (file:line into the reference tree).  All buffers are caller-owned,
 * plain pointers and sizes; no Python, torch or C++ types cross the boundary.  Functions
 * return 0 on success or a negative GAT_ERR_* code; gat_last_error() gives the text.
 * One gat_ctx per host thread; a ctx is bound to one HIP device and one HIP stream.
 *
 * There is NO CPU fallback behind this ABI: every entry point that computes runs HIP kernels
 * and fails with GAT_ERR_DEVICE when no gfx950 device is usable.
 */
#ifndef GAT_MI355_H
#define GAT_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == gat/SegmentList.pxd:31-38  struct Segment { Position start; Position end; }, half-open */
typedef struct { uint32_t start, end; } gat_segment;

typedef struct gat_ctx gat_ctx;
typedef struct gat_problem gat_problem;
typedef struct gat_annotations gat_annotations;

#define GAT_OK 0
#define GAT_ERR_VALUE (-1)      /* reference raises ValueError (gat/SegmentList.pyx:1170-1182)      */
#define GAT_ERR_ASSERT (-2)     /* reference raises AssertionError (gat/Engine.pyx:535-536, :645)   */
#define GAT_ERR_CAPACITY (-3)   /* a caller buffer or a device slab was too small                  */
#define GAT_ERR_MEMORY (-4)
#define GAT_ERR_DEVICE (-5)     /* HIP error / no usable gfx950 device                             */
#define GAT_ERR_ARG (-6)

/* counter ids == the classes of gat/Engine.pyx:1417-1472 (Counter*.name) */
#define GAT_COUNTER_NUCLEOTIDE_OVERLAP 0     /* CounterNucleotideOverlap        :1417 */
#define GAT_COUNTER_NUCLEOTIDE_DENSITY 1     /* CounterNucleotideDensity        :1428 */
#define GAT_COUNTER_SEGMENT_OVERLAP 2        /* CounterSegmentOverlap           :1443 */
#define GAT_COUNTER_SEGMENT_MIDOVERLAP 3     /* CounterSegmentMidpointOverlap   :1450 */
#define GAT_COUNTER_ANNOTATION_OVERLAP 4     /* CounterAnnotationOverlap        :1458 */
#define GAT_COUNTER_ANNOTATION_MIDOVERLAP 5  /* CounterAnnotationMidpointOverlap :1465 */
#define GAT_NUM_COUNTERS 6

/* samplers */
#define GAT_SAMPLER_ANNOTATOR 0   /* SamplerAnnotator: place until the workspace overlap matches (default)   */
#define GAT_SAMPLER_SEGMENTS 1    /* SamplerSegments: len(segments) placements, no consolidation; the lists are */
                                  /* normalized only by fromIsochores, so counters need isochore keys           */
#define GAT_SAMPLER_SHIFT 2       /* SamplerShift(radius, extension) (gat/Engine.pyx:998-1111): every working   */
                                  /* segment moved within a window around itself; per-unit streams only         */
#define GAT_SAMPLER_GLOBAL_PERMUTATION 3  /* SamplerGlobalPermutation (gat/Engine.pyx:1234-1386): the working       */
                                  /* segments' lengths shuffled, random gaps, laid into the workspace extended  */
                                  /* by them from a random shift; Python's random; per-unit streams only        */
#define GAT_SAMPLER_LOCAL_PERMUTATION 4   /* SamplerLocalPermutation (gat/Engine.pyx:1117-1229): per workspace piece,   */
                                  /* the lengths of getOverlappingSegments' set shuffled, random gaps, laid over */
                                  /* [0, piece end) from a random shift (what the reference computes: its        */
                                  /* min() / max() return 0); the pieces' outputs united by normalize(); a unit  */
                                  /* is active when some piece has a working segment; free < 0 in a piece or a   */
                                  /* coordinate beyond 2^31 - 1 (where the reference raises): GAT_ERR_ASSERT;    */
                                  /* Python's random; per-unit streams only                                     */
#define GAT_SAMPLER_BRUTE_FORCE 5  /* SamplerBruteForce(bucket_size, nbuckets, ntries_inner, ntries_outer)          */
                                  /* (gat/Engine.pyx:746-871): SamplerAnnotator's draws, a segment kept only if   */
                                  /* it overlaps no earlier one, until the overlaps with the workspace add up to  */
                                  /* segments.sum() exactly; ntries_inner rejections in a row restart the list    */
                                  /* (the stream goes on), ntries_outer passes without success fail the call with */
                                  /* GAT_ERR_VALUE "sampling did not converge", gat_last_error naming the first   */
                                  /* (sample, unit); numpy's stream; per-unit streams only                        */
#define GAT_SAMPLER_CIRCULAR 6    /* SamplerCircular (no counterpart in the reference): the  */
                                  /* working segments cut to the workspace, rotated as a whole by one offset      */
                                  /* r = randint(0, Wsum) along the workspace with its gaps taken out -- every      */
                                  /* length and every gap between segments kept -- and cut at the workspace       */
                                  /* borders and the wrap, nothing united afterwards; a problem without tracks    */
                                  /* and isochore keys takes coordinates up to 2^32 - 1; numpy's stream; per-unit  */
                                  /* streams only                                                                 */
#define GAT_SAMPLER_UNIVERSE 7    /* SamplerUniverse (no counterpart in the reference): the  */
                                  /* unit's workspace pieces are the universe of candidate regions; k of the m    */
                                  /* pieces share a base with a segment, and a sample is k pieces chosen          */
                                  /* uniformly without replacement (Floyd's algorithm on the smaller side), each  */
                                  /* whole, in genome order, nothing united or cut; a unit whose table of m mark  */
                                  /* bits is beyond the context's LDS is refused at gat_problem_create with       */
                                  /* GAT_ERR_ARG; numpy's stream; per-unit streams only                           */

/*
 * Flat description of what gat.computeSample (gat/__init__.py:494-591) walks for one segment
 * track: the isochore units in list(segs.keys()) order (:531), their contig after
 * IntervalDictionary.fromIsochores (gat/Engine.pyx:2857-2876), and the contig-level
 * annotations / workspace the counters see (:580-587).  All pointers are HOST pointers and are
 * only read during gat_problem_create.  Every list must be normalized (sorted, disjoint,
 * non-empty segments: gat/SegmentList.pyx:697) and all coordinates must be < 2^31 (the
 * reference's int32 lmin/lmax, gat/SegmentList.pyx:68-77, are order-preserving only there).
 * The samplers that draw lengths (GAT_SAMPLER_ANNOTATOR, _SEGMENTS, _BRUTE_FORCE) also need the END of every segment they
 * can place to be a coordinate: for every active unit, last workspace end + Lmax - 1 <= 2^31 - 1, Lmax = the longest
 * length the unit's histogram can return (the largest bucket it can draw x bucket size, + bucket size - 1 when the
 * bucket size is > 1: with buckets a drawn length can exceed every segment of the unit; of two or more working segments
 * the last rank is never drawn, gat/Engine.pyx:420, so that bucket is the second longest segment's).  gat_problem_create refuses a unit outside this
 * domain with GAT_ERR_ARG; past it the reference itself computes on wrapped int32 values.
 */
typedef struct {
  int32_t n_units;              /* isochore keys, reference order                               */
  const gat_segment* segs;      /* per-unit segment lists, concatenated                         */
  const int64_t* seg_off;       /* n_units+1                                                    */
  const gat_segment* ws;        /* per-unit workspace lists, concatenated                       */
  const int64_t* ws_off;        /* n_units+1                                                    */
  const int32_t* unit_contig;   /* n_units: contig index, or -1 for a unit computeSample skips  */
  int32_t n_contigs;            /* contigs in list(sample.keys()) order after fromIsochores     */
  int32_t merge_contigs;        /* 1 if keys are "contig.isochore": fromIsochores merges(0)     */
  int32_t n_tracks;             /* annotation tracks                                            */
  const gat_segment* annos;     /* [track][contig] lists, concatenated                          */
  const int64_t* anno_off;      /* n_tracks*n_contigs+1                                         */
  const int64_t* cws_nseg;      /* n_contigs: len(contig_workspace[contig]) (Engine.pyx:1437)   */
  uint32_t bucket_size;         /* SamplerAnnotator(bucket_size, nbuckets): gat/Engine.pyx:498  */
  int32_t nbuckets;
  int32_t sampler;              /* GAT_SAMPLER_ANNOTATOR (gat/Engine.pyx:445), GAT_SAMPLER_SEGMENTS (:653), GAT_SAMPLER_SHIFT (:998), GAT_SAMPLER_GLOBAL_PERMUTATION (:1234), GAT_SAMPLER_LOCAL_PERMUTATION (:1117), GAT_SAMPLER_BRUTE_FORCE (:746), GAT_SAMPLER_CIRCULAR or GAT_SAMPLER_UNIVERSE */
  /* Optional (all 0 / NULL: annos / anno_off are the [track][contig] lists above).  With anno_group set, the caller hands
   * over the annotation lists as it holds them -- one per (track, isochore key), the `annotations` argument of
   * UnconditionalSampler.sample (gat/__init__.py:704) -- and the library forms computeSample's contig_annotations itself
   * (gat/__init__.py:716-718 -> IntervalDictionary.fromIsochores, gat/Engine.pyx:2857-2876: the lists of a contig
   * concatenated and, when merge_contigs, sorted and merge(0)d), on host threads: */
  int64_t n_anno_lists;         /* number of lists; list l = annos[anno_off[l] .. anno_end[l])                       */
  const int64_t* anno_end;      /* n_anno_lists, or NULL: anno_off has n_anno_lists + 1 entries (CSR)                 */
  const int32_t* anno_group;    /* n_anno_lists: track * n_contigs + contig of the list's key, or -1 (its contig has   */
                                /* no unit that computeSample samples: the counters never see it)                      */
  /* Optional: the annotation side as an object made before (gat_annotations_create) -- the reference passes the SAME
   * annotations to the sampling of every segment track (gat/__init__.py:971-1010); a host that loops over tracks builds
   * their tables once.  n_tracks / n_contigs / merge_contigs must be the object's; annos / anno_* above are ignored. */
  const gat_annotations* annotations;
  /* GAT_SAMPLER_SHIFT only (ignored otherwise): SamplerShift(radius, extension) -- the window around a segment is
   * extension // 2 on either side of its midpoint when extension != 0, else floor(length * radius / 2).  Both must be
   * >= 0 (GAT_ERR_VALUE): the reference's unsigned casts give a negative value no meaning. */
  double shift_radius;
  int32_t shift_extension;
  /* GAT_SAMPLER_BRUTE_FORCE only (ignored otherwise): SamplerBruteForce(ntries_inner, ntries_outer); 0: the reference's
   * defaults, 100 and 10; negative: GAT_ERR_VALUE. */
  int32_t brute_ntries_inner;
  int32_t brute_ntries_outer;
} gat_problem_desc;

/* The annotation side of gat_problem_desc by itself: the tracks' lists per contig -- [track][contig] CSR, or with
 * anno_group one list per (track, isochore key) that the library groups as IntervalDictionary.fromIsochores does
 * (gat/Engine.pyx:2857-2876) -- for the contigs, IN THE ORDER, of the problems that will count against it. */
typedef struct {
  int32_t n_tracks;
  int32_t n_contigs;
  int32_t merge_contigs;
  const gat_segment* annos;
  const int64_t* anno_off;      /* n_tracks*n_contigs+1, or per list (see anno_end)                                   */
  int64_t n_anno_lists;         /* with anno_group: number of lists                                                    */
  const int64_t* anno_end;
  const int32_t* anno_group;
  double mean_segment_length;   /* of the segments that will be counted against them, 0 if unknown: picks the form of  */
                                /* the merged index (speed only, never a result)                                       */
  int32_t flags;                /* 0 or an OR of GAT_ANNOTATIONS_ASYNC, GAT_ANNOTATIONS_NUCLEOTIDE_ONLY                 */
} gat_annotations_desc;

/* gat_annotations_create returns at once and a thread of the library builds the tables (its own stream and staging
 * buffer): the arrays of the desc must stay valid until gat_annotations_wait -- or a gat_wait of a call counted against the
 * object -- has returned.  A problem made against such an object can be sampled straight away: gat_sample_and_count_enqueue
 * puts the sampler's kernels on the stream and the count kernels follow when the tables are there (at the latest in
 * gat_wait).  Errors of the build are reported by the call that first needs the tables.  Honoured where the shape alone
 * tells which count kernel will run (four tracks or more); otherwise the build is synchronous. */
#define GAT_ANNOTATIONS_ASYNC 1
/* The object will only be counted against with the nucleotide counters (GAT_COUNTER_NUCLEOTIDE_OVERLAP / _DENSITY: what
 * gat.run() does unless the caller asked for segment or annotation counters).  Where the merged index of all tracks is built
 * (four tracks or more, or lists beyond the per-track kernel's LDS tile) the per-track tables -- starts / ends / running
 * lengths and the position grids, a third of the build -- are left out; gat_sample_and_count with any other counter on a
 * problem made against such an object fails with GAT_ERR_ARG.  Ignored where no merged index is built. */
#define GAT_ANNOTATIONS_NUCLEOTIDE_ONLY 2

/* per-call statistics of gat_sample_and_count / gat_sample (device time from HIP events on the
 * ctx stream; counts summed over all (sample, unit) work units of the call).  ms_total and ms_count_main are always
 * measured; the other ms_* fields -- an event behind every kernel of the sampler, 2 % of a 10 000-sample call and 6 % of
 * a 1 250-sample one -- only after gat_ctx_set_kernel_times(ctx, 1), else 0 */
typedef struct {
  float ms_sampler;             /* placement + consolidation kernel                             */
  float ms_contig;              /* fromIsochores kernel (0 when keys carry no isochore)         */
  float ms_count;               /* overlap-count kernel(s)                                      */
  float ms_total;               /* whole call on the stream                                     */
  int64_t n_placed;             /* segments placed (sls.sample calls kept, gat/Engine.pyx:628)  */
  int64_t n_draws;              /* raw MT19937 outputs consumed                                 */
  int64_t n_sampled_segments;   /* contig-level segments returned (gat_sample only)               */
  int64_t n_unsuccessful;       /* sum of nunsuccessful_rounds (gat/Engine.pyx:570-572)         */
  int64_t n_retried;            /* work units redone with a larger slab                         */
  int64_t n_full_units;         /* work units run without the lane-parallel front end           */
  float ms_count_main;          /* the dominant count kernel alone (see count_kernel)             */
  float ms_rng;                 /* split of ms_sampler: k_rng (MT19937 rows)                      */
  float ms_place;               /*   k_place (placement up to the first consolidation)            */
  float ms_merge;               /*   first consolidation: k_consolidate, or k_merge_big for long lists */
  float ms_tail;                /*   everything behind it: k_tail + k_finalize + k_sampler        */
  int32_t count_kernel;         /* GAT_COUNT_KERNEL_* the call used for the overlap counters      */
  float ms_ktail;               /*   of ms_tail: k_tail (the loop's tail, one stream per lane)    */
  float ms_finalize;            /*   of ms_tail: k_finalize (merged list + extras -> final list)   */
  int64_t n_tail_units;         /* work units finished by k_tail, or (long lists) carried through their placement rounds
                                   by k_tail_big before k_sampler resumed them                        */
  int64_t lists_from_records;   /* != 0: no final unit lists were written; their consumer (k_contig or k_count_seg) took
                                   the merged lists and k_tail's records                              */
  int64_t n_index_entries;      /* k_count_merged: 4-byte words of index its scans read (grid cells, entries), and ...  */
  int64_t n_index_lookups;      /*   ... the sample segments it looked up: what the kernel's byte model is made of       */
  int64_t n_batches;            /* batches the call was cut into (the scratch budget decides how many samples one holds)   */
  int64_t merged_form;          /* k_count_merged: how its scans fetched the index: 8 blocks of eight entries, 2 pairs,    */
                                /* 1 the grid cell's record (its first two entries) + pairs; 0: the kernel did not run     */
  int64_t n_resumed_units;      /* work units whose pre-generated random rows ran out and whose stream went on from the     */
                                /* generator moved up to its position (instead of a run in full: n_full_units)              */
  int64_t n_straddle_candidates; /* isochore problems whose contig lists were only concatenated (nucleotide counters; k_contig<., true>):  */
                                /* segments with a workspace boundary in their cells, of units that have a segment reaching out of   */
                                /* their workspace -- what k_units_overlap looked at; 0: the sorted, merged contig lists were made   */
  int64_t n_unit_overlaps;      /* ... and the overlaps between different units' segments it took off the sums again -- what      */
                                /* IntervalDictionary.fromIsochores' merge(0) unites (gat/Engine.pyx:2857-2876)                   */
  int64_t kernel_times;         /* the ms_* split of the sampler's kernels: 1 recorded, 0 not asked for (gat_ctx_set_kernel_times),   */
                                /* -1 asked for but NOT recorded -- the events exist once per context and another problem's timed  */
                                /* call was in flight (gat_amd.run() keeps two segment tracks' calls in flight): the fields read 0 */
  int64_t n_queued_units;       /* work units k_tail (lists of up to 1 024 segments) or k_resume_big (longer ones) left to     */
                                /* k_sampler's queue: a wave each, the slow way (0 when neither ran: k_sampler took every unit)  */
  int64_t n_empty_windows;      /* GAT_SAMPLER_SHIFT: segments whose window held no workspace base -- the reference's         */
                                /* randint(0, 0) raises inside getRandomPosition, which returns 0; the direction is still     */
                                /* drawn and the segment contributes nothing (gat/SegmentList.pyx:902-917)                     */
  int64_t n_restarts;           /* GAT_SAMPLER_BRUTE_FORCE: outer passes beyond a work unit's first, summed over the call      */
  int64_t n_unconverged;        /* ... and work units that used up ntries_outer passes: the call fails with GAT_ERR_VALUE (its */
                                /* statistics are still written)                                                               */
} gat_stats;

#define GAT_COUNT_KERNEL_NONE 0
#define GAT_COUNT_KERNEL_SEG 1      /* k_count_seg: annotation tiles in LDS, sample segments looked up   */
#define GAT_COUNT_KERNEL_SWAP 2     /* k_count_swap: sample list indexed in LDS, annotation tracks streamed */
#define GAT_COUNT_KERNEL_MERGED 3   /* k_count_merged: one look-up per sample segment in a merged index of all tracks */

/* What the count stage launched last on a context: the newest batch of a gat_sample_and_count* call, or the LAST list of a
 * gat_count_lists / gat_count_list_ranges call (one launch per list).  For tests and diagnosis: which of the kernels the sizes
 * and the GAT_COUNT_* / GAT_MERGED_* options led to.  All zero when nothing was launched. */
typedef struct gat_count_report {
  int32_t kernel;             /* GAT_COUNT_KERNEL_*: what served the segment-side counters                              */
  int32_t staged;             /* k_count_seg: 1 the track tile's lists staged in LDS, 0 read from global memory         */
  int32_t hits;               /* k_count_seg: 1 the variant that also counts segment-overlap / segment-midoverlap        */
  int32_t patch;              /* k_count_seg / k_count_merged: 1 the lists read as (merged list, k_tail's record)         */
  int32_t tracks_per_block;   /* k_count_seg: tracks of a tile as launched, else 0                                       */
  int32_t samples_per_block;  /* k_count_seg / k_count_merged: samples of a workgroup as launched, else 0                */
  int32_t merged_form;        /* k_count_merged: how a scan fetches the index, 8, 2 or 1; 0: it did not run              */
  int32_t anno_kernel;        /* the annotation-side counters: 0 none, 1 k_count_anno_idx, 2 k_count_anno               */
} gat_count_report;
#define GAT_COUNT_ANNO_NONE 0
#define GAT_COUNT_ANNO_IDX 1
#define GAT_COUNT_ANNO_PLAIN 2

/* What the sampler stage planned for the newest batch of a call on a context: the plan's flags, and per size class of the
 * launch order what the long-list chain and the split path were launched with (SamplerAnnotator / SamplerSegments; the
 * samplers that run one kernel per unit report sampler_variant -1 and nothing else).  Host bookkeeping for tests and
 * diagnosis: no launch depends on it, and what the kernels decided per (sample, unit) is in gat_stats.  All zero before the
 * first batch. */
#define GAT_SAMPLER_REPORT_CLASSES 8
typedef struct gat_sampler_class_report {
  int32_t first;              /* the class's first launch position                                                      */
  int32_t merge_ccap;         /* k_merge_big: segments its LDS holds for the class, 0: not launched for the class      */
  int32_t merge_buckets;      /* k_merge_big: the counting sort's buckets at most, 0: not launched                     */
  int32_t merge_form;         /* k_merge_big: list elements per thread in registers, 8, 16 or 24; 0 the two-pass form; */
                              /* -1: not launched for the class                                                        */
  int32_t consolidate_ccap;   /* k_consolidate: segments the LDS of the launch that covers the class holds, 0: none    */
} gat_sampler_class_report;
typedef struct gat_sampler_report {
  int32_t huge;               /* lists beyond LDS: worked on in global memory                                           */
  int32_t split;              /* the split path ran: k_consolidate, k_tail (, k_finalize) in front of k_sampler          */
  int32_t long_lists;         /* k_sampler's code for lists beyond the wave's bucket sorts                               */
  int32_t merge_big;          /* k_merge_big launched over the long units ...                                            */
  int32_t tail_big;           /* ... k_tail_big behind it ...                                                            */
  int32_t resume_big;         /* ... k_resume_big behind that ...                                                        */
  int32_t long_queue;         /* ... and k_sampler working off k_queue_rest's queue                                      */
  int32_t resume_virtual;     /* k_resume_big<true>: the log left behind the merged list (counts through the merged index) */
  int32_t tree;               /* the TREE instantiations: some workspace has more segments than the register loop takes  */
  int32_t big_buckets;        /* no k_merge_big: buckets of k_sampler's own counting sort of lists above 1 024, 0: none  */
  int32_t n_long;             /* launch positions [0, n_long) are long units                                             */
  int32_t sampler_variant;    /* k_sampler / k_serial: 0..3 SamplerAnnotator (+1 trees, +2 long lists), 4 / 5            */
                              /* SamplerSegments, 6 / 7 lists in global memory, 8 variant 0 at five waves per SIMD       */
  int32_t n_classes;          /* size classes of the launch order (the first GAT_SAMPLER_REPORT_CLASSES are recorded)    */
  gat_sampler_class_report cls[GAT_SAMPLER_REPORT_CLASSES];
} gat_sampler_report;

/* ---- context ---------------------------------------------------------------------------- */
/* device_id: HIP device ordinal.  stream: a hipStream_t to run on (e.g. a torch stream's handle; the default stream is
 * named by hipStreamLegacy, (hipStream_t)1 -- its own handle is NULL) or NULL to create a private non-blocking one. */
int gat_ctx_create(gat_ctx** out, int device_id, void* stream);
void gat_ctx_destroy(gat_ctx* ctx);
const char* gat_last_error(const gat_ctx* ctx);      /* ctx may be NULL: last error of the thread */
const char* gat_version(void);
int gat_ctx_synchronize(gat_ctx* ctx);
/* The tuning / testing knobs (GAT_*) of a context.  None is needed for normal use.  A knob's value is the
 * context's own (set here: value "" = not set, whatever the environment says; NULL = back to the process's), else the process's
 * environment variable of that name AS IT WAS when the library first looked (one snapshot: nothing reads the environment on a
 * call's path, and two host threads with a context each do not see each other's settings).  All of them are read at once, at
 * three moments: when a problem is created, when annotation tables are created (an asynchronous build works under the values
 * of its creation), and at the top of a call (every batch of the call, the ones gat_wait enqueues too).  A set_option acts on
 * the problems, tables and calls started after it; it is safe at any time from the thread that owns the context.
 * gat_ctx_get_option returns a copy kept per calling thread: the pointer is valid until that thread's next gat_ctx_get_option,
 * whatever is set meanwhile. */
int gat_ctx_set_option(gat_ctx* ctx, const char* key, const char* value);
const char* gat_ctx_get_option(const gat_ctx* ctx, const char* key);   /* NULL: not set */
/* the hipStream_t the context's work is enqueued on (the one given to gat_ctx_create, or its private stream): a host that
 * runs other work on the device -- a collective over the count matrix, a copy -- orders it against the library's with
 * events on this stream instead of synchronising the device */
void* gat_ctx_stream(const gat_ctx* ctx);
/* Call lanes (GAT_CALL_LANES, default 2, at most 4; below 2: none).  A call enqueued with gat_sample_and_count_enqueue while a
 * call of ANOTHER problem of the context is in flight runs on a stream of the library's own, beside that call.  Towards the
 * caller's stream it is ordered both ways: its count kernels -- its first access to the caller's count matrix -- wait for what
 * was on the caller's stream at the enqueue, and the caller's stream waits for the call before it takes up what is put on it
 * after the enqueue.  Its sampler kernels touch only the problem's own scratch and start at once.
 * gat_call_lane_for is the rule itself, a pure function (no device): the lane (0 .. n_lanes - 1) a call takes, or -1 for the
 * context's stream.  lane_busy: n_lanes flags, a call in flight runs on that lane; others_in_flight: calls of other problems
 * in flight on the context.  Synchronous entry points, calls with per-kernel timing and calls with a serial MT19937 state
 * stay on the context's stream; so does a call with nothing else in flight. */
int gat_call_lane_for(int n_lanes, int asynchronous, int timed, int serial_state, int others_in_flight, const int32_t* lane_busy);
/* per-kernel device times in gat_stats (see there) on / off; off by default.  GAT_KERNEL_TIMES=1 in the environment
 * switches them on for every context. */
int gat_ctx_set_kernel_times(gat_ctx* ctx, int on);

/* device memory helpers so a ctypes host needs no other HIP binding */
int gat_dev_alloc(gat_ctx* ctx, void** out, size_t bytes);
int gat_dev_free(gat_ctx* ctx, void* p);
int gat_memcpy_d2h(gat_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int gat_memcpy_h2d(gat_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);

/* ---- problem ---------------------------------------------------------------------------- */
/* Uploads the inputs once and hoists what SamplerAnnotator.sample recomputes on every call
 * (gat/Engine.pyx:543-565: filter, ltotal, getLengthDistribution, both sampler CDFs).
 * Returns GAT_ERR_VALUE where the reference's first sample() would raise ValueError.
 * Limits (GAT_ERR_CAPACITY beyond them): 2^24 workspace segments per unit, 2^31 segments per sample; no limit on
 * the number of units or contigs.  There is no limit on the segments of a unit: lists that do not fit
 * on-chip memory are worked on in device memory.  GAT_ERR_ARG: a coordinate >= 2^31, or -- SamplerAnnotator,
 * SamplerSegments, SamplerBruteForce; the per-unit and the serial stream alike -- an active unit whose last workspace
 * end + Lmax - 1 exceeds 2^31 - 1 (see gat_problem_desc; gat_last_error names the unit, the workspace end and Lmax).
 * Units without a working segment or a workspace are not looked at. */
int gat_problem_create(gat_ctx* ctx, const gat_problem_desc* desc, gat_problem** out);
void gat_problem_destroy(gat_problem* p);

/* Uploads the annotation tracks and builds what the counters look them up in (SoA lists + position grids, the merged
 * index of all tracks): the part of gat_problem_create that does not depend on the segment track.  Problems created with
 * desc->annotations = this object share it; it may be destroyed before them (it lives until the last one is gone). */
int gat_annotations_create(gat_ctx* ctx, const gat_annotations_desc* desc, gat_annotations** out);
int gat_annotations_wait(gat_ctx* ctx, gat_annotations* a);      /* an asynchronous build has finished; its error, if any */
void gat_annotations_destroy(gat_annotations* a);

/* ---- the batch seam ---------------------------------------------------------------------
 * Replaces UnconditionalSampler.sample / computeSamples / computeSample
 * (gat/__init__.py:654-778, :494-591) for samples [sample_begin, sample_end):
 * per sample, every unit is sampled (SamplerAnnotator.sample, gat/Engine.pyx:515-646),
 * units are re-combined per contig (fromIsochores) and every counter x annotation track is
 * evaluated and summed over contigs.
 *
 * Random streams ("per-unit" contract): work unit (sample s, unit u) draws from
 * numpy's legacy RandomState seeded with (seed + s*n_units + u) mod 2^32, i.e. exactly what
 * numpy.random.seed(that) followed by the reference's sampler.sample() consumes.  Results do
 * not depend on how samples are split over calls, streams or GPUs.
 *
 * counts_dev: DEVICE pointer to n_counters*n_tracks*(sample_end-sample_begin) 8-byte slots laid
 * out [counter][track][sample]; int64 for the integer counters, IEEE double for
 * nucleotide-density.  Work is enqueued on the ctx stream; the call returns after the
 * kernels have completed and per-unit status words have been checked.  A context may be destroyed before the problems
 * made on it: it lives until the last of them is gone. */
int gat_sample_and_count(gat_ctx* ctx, gat_problem* p,
                         const int32_t* counter_ids, int n_counters,
                         uint32_t seed, int64_t sample_begin, int64_t sample_end,
                         void* counts_dev, gat_stats* stats /* nullable */);

/* The same call in two halves, for a host that has work of its own to do while the device samples (gat.run computes the
 * observed counts, gat/__init__.py:933-940, and the sizes of its result rows, :1000-1068, around the sampling; the
 * reference's process pool -- map_async, gat/__init__.py:681-700 -- is asynchronous in the same way).
 * gat_sample_and_count_enqueue validates the arguments, enqueues the call's batches (up to 8 ahead; on the ctx stream or a call lane, below) and
 * returns; counts_dev must stay valid and untouched until gat_wait.  gat_wait(ctx, p, stats) blocks until the batches have
 * completed, checks their status words -- a batch that has to be repeated (a unit's region of the slab overflowed) is
 * repeated in here, with everything that was enqueued behind it -- and reports what gat_sample_and_count would have
 * (GAT_ERR_ASSERT where the reference's sampler asserts, :645).  One call in flight per problem; several problems of one
 * context may each have one (their kernels run side by side on the context's call lanes, gat_call_lane_for; with
 * GAT_CALL_LANES=1 one behind the other on the context's stream; gat_wait waits for the end of ITS call
 * -- an event behind its last batch --, not for a stream: what another problem has enqueued keeps running
 * while the host reads the results and enqueues the next call).  gat_problem_destroy drops a call in flight.  gat_sample_and_count(...) == enqueue + wait. */
int gat_sample_and_count_enqueue(gat_ctx* ctx, gat_problem* p,
                                 const int32_t* counter_ids, int n_counters,
                                 uint32_t seed, int64_t sample_begin, int64_t sample_end, void* counts_dev);
int gat_wait(gat_ctx* ctx, gat_problem* p, gat_stats* stats /* nullable */);

/* Sampler only: replaces sampler.sample() + sample.fromIsochores() (gat/__init__.py:541, :563)
 * for a range of samples and returns the contig-level lists to the HOST:
 * off_host has (sample_end-sample_begin)*n_contigs+1 entries, segments of (sample i, contig c)
 * are out_host[off[i*n_contigs+c] .. off[i*n_contigs+c+1]).  GAT_ERR_CAPACITY if cap is too
 * small (off_host[last] then holds the required size). */
int gat_sample(gat_ctx* ctx, gat_problem* p, uint32_t seed,
               int64_t sample_begin, int64_t sample_end,
               gat_segment* out_host, int64_t cap, int64_t* off_host, gat_stats* stats);

/* The same at unit level: what sampler.sample(segs[isochore], workspace[isochore]) returned for every (sample, unit)
 * before fromIsochores (gat/__init__.py:541; the lists --output-samples-pattern writes, :549-559).  off_host has
 * (sample_end-sample_begin)*n_units+1 entries; units computeSample skips are empty. */
int gat_sample_units(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                     int64_t sample_begin, int64_t sample_end,
                     gat_segment* out_host, int64_t cap, int64_t* off_host, gat_stats* stats);

/* Where a null model puts its segments: per-bin coverage of the sampled lists, summed over the samples
 * [sample_begin, sample_end), formed on the device where the sampler leaves the lists.  Stands in for
 * computeSegmentDensityProfile (test/validate_randomization.py:212-247: per-position counts of the samples and histograms
 * of the segments' starts and ends, by per-base loops on the host).  Bin b of contig c is [b * bin_size, (b + 1) * bin_size),
 * contig c has n_bins[c] = bin_off[c + 1] - bin_off[c] of them.  Every segment [s, e), e > s, of every contig-level list
 * (sample i, contig c) -- exactly the lists gat_sample returns, drawn from the same per-unit streams -- adds
 *     bases[bin_off[c] + b] += |[s, e) n bin b|                    for b < n_bins[c]
 *     outside[c]            += |[s, e) n [n_bins[c] * bin_size, inf)|
 *     starts[bin_off[c] + b] += 1 where s lies in bin b,  ends[bin_off[c] + b] += 1 where e - 1 does
 * (starts and ends beyond the last bin are dropped).  Lists need be neither sorted nor disjoint (SamplerSegments without
 * isochore keys returns neither): overlapping segments count with their multiplicity, and for every contig
 * sum(bases) + outside == the summed lengths of its lists.  All sums are exact 64-bit integers and do not depend on how the
 * sample range is cut into batches or calls.  Where the clipping differs from the reference: that clamps every segment to
 * [0, workspace.max()); here the caller's n_bins is the extent and `outside` reports what lies beyond it.
 * bin_off: n_contigs + 1 entries (HOST), bin_off[0] >= 0, not decreasing; bases_host / starts_host / ends_host:
 * bin_off[n_contigs] entries each (HOST; starts_host / ends_host may be NULL: not wanted); outside_host: n_contigs.
 * Synchronous, like gat_sample.  GAT_ERR_ARG: a NULL ctx / p / bin_off / bases_host / outside_host, bin_size outside
 * [1, 2^31], a decreasing bin_off, sample_end < sample_begin, a call in flight on the problem.  An empty sample range gives
 * zeros.  The sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's GAT_ERR_VALUE "sampling did not
 * converge").  Per-unit streams only.  GAT_COVERAGE_WINDOW_BINS / GAT_COVERAGE_SAMPLES_PER_BLOCK (context options): the
 * bins and samples a workgroup of k_coverage takes; neither changes a result. */
int gat_sample_coverage(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                        int64_t sample_begin, int64_t sample_end,
                        int64_t bin_size, const int64_t* bin_off,
                        int64_t* bases_host, int64_t* starts_host, int64_t* ends_host,
                        int64_t* outside_host, gat_stats* stats /* nullable */);

/* How lists of segments sit in a workspace: the sums behind SegmentsSummary.update / IO.outputMetrics (gat/IO.py:331-454;
 * the reference's --output-stats=segment_metrics / sample_metrics), formed on the device by k_metrics.  For a list L and
 * the normalized pieces W of its group -- sorted, disjoint; adjacent pieces stay two pieces, as normalize leaves them --
 * every segment [s, e) of L has  lo = the first piece with end > s,  hi = the last piece with start < e,
 * k = max(0, hi - lo + 1), and adds to eight int64 words (GAT_METRICS_WORDS), in this order:
 *     n               1
 *     bases           e - s
 *     pairs           k
 *     inter           |[s, e) n W|
 *     touched         e - s where k > 0
 *     outside_pieces  1 where k == 0, else [s < W[lo].start] + [e > W[hi].end] + the number of j in lo+1..hi with
 *                     W[j].start > W[j-1].end
 *     tail_n          1 where s > M, M = the largest start of a segment of L with k > 0 (-1: none has)
 *     tail_bases      e - s where s > M
 * The first six are what L and W say; the last two are what the reference's subtract never reaches: its merge-join ends with
 * the last piece of the intersection, so the segments behind the last one that touches W (all of them with k == 0; every
 * segment where none touches W) are missing from its result.  For a sorted, disjoint L: n = len(L), bases = L.sum(),
 * pairs = len(L.filter(W).intersect(W)), inter = its sum(), touched = L.filter(W).sum(), and L.subtract(that intersection)
 * has outside_pieces - tail_n segments of bases - inter - tail_bases bases (gat/SegmentList.pyx:1204-1285, :1401-1549).  Lists need be neither sorted nor disjoint (SamplerSegments without
 * isochore keys returns neither): the per-segment form is then the definition, overlapping segments count with their
 * multiplicity.  All sums are exact 64-bit integers (the reference's Position accumulator wraps at 2^32).  A word has one
 * owner on the device and is written once: results are reproducible.  GAT_METRICS_LDS_PIECES (context option): how many
 * pieces of a group the kernel's searches find in LDS before they go to global memory; it changes no result.
 *
 * gat_list_metrics: caller-provided lists.  lists: n_lists * n_groups segment lists (HOST, CSR via list_off, n_lists *
 * n_groups + 1 entries), list l of group g at index l * n_groups + g; ws / ws_off: the n_groups piece lists (HOST, CSR,
 * n_groups + 1 entries); out_host: [n_lists][n_groups][8].  Synchronous.  GAT_ERR_ARG: a NULL ctx / list_off / ws_off /
 * out_host (lists / ws may be NULL where they hold nothing), negative counts, a decreasing offset, a segment that ends
 * before it starts, a piece list that is not normalized (gat_last_error names the group). */
#define GAT_METRICS_WORDS 8
int gat_list_metrics(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                     const gat_segment* ws, const int64_t* ws_off, int32_t n_groups, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_metrics behind every batch that passed its checks, reading
 * the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed and
 * range (per-unit streams only).  ws / ws_off: the pieces each contig's samples are measured against (HOST, CSR,
 * n_contigs + 1 entries, in the problem's contig order); out_host: [sample][contig][8], sample_end - sample_begin samples.
 * Synchronous, like gat_sample.  Results do not depend on how the range is cut into batches or calls.  GAT_ERR_ARG: a NULL
 * ctx / p / ws_off / out_host, sample_end < sample_begin, a decreasing ws_off, a piece list that is not normalized, a call
 * in flight on the problem.  An empty sample range writes nothing.  The sampler's errors pass through (GAT_ERR_ASSERT;
 * SamplerBruteForce's GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_metrics(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                       int64_t sample_begin, int64_t sample_end,
                       const gat_segment* ws, const int64_t* ws_off,
                       int64_t* out_host, gat_stats* stats /* nullable */);

/* How far the intervals of one list lie from the nearest interval of another: the two counters the reference's to-do list
 * names and never built (doc/contents.rst:78-81, "Closest distance of segment to annotation" / "Closest distance of annotation
 * to segment"), formed on the device by k_distance.  T is a normalized list of K >= 1 intervals -- sorted by start, pairwise
 * disjoint, every interval with end > start; adjacent intervals allowed -- and Q = [s, e) a query with e > s.  With
 * j = the first index with T[j].end > s (K: none):  T[j].start < e: the two share a base, d = 0;  else d = the smaller of
 * T[j].start - e + 1 (where j < K) and s - T[j - 1].end + 1 (where j > 0).  This is the convention of `bedtools closest -d`:
 * bookended intervals are at distance 1, a one-base overlap at 0.  A list of queries is compared with a list T group by
 * group (contig by contig) and adds to four int64 words (GAT_DISTANCE_WORDS), summed over the groups, in this order:
 *     n      queries with e > s on groups where T is not empty
 *     sum    d, over those queries
 *     near   how many of them have d <= max_distance
 *     none   queries with e > s on groups where T is empty: they have no neighbour and add nothing else
 * Queries with e <= s are skipped everywhere.  The queries need be neither sorted nor disjoint (SamplerSegments without
 * isochore keys returns neither): every query counts on its own.  direction: GAT_DISTANCE_SEGMENT_TO_ANNOTATION -- the queries
 * are a segment list, T an annotation track; GAT_DISTANCE_ANNOTATION_TO_SEGMENT -- the queries are the track's intervals and T
 * the segment list, which must then be normalized (GAT_ERR_ARG where it is not, never a wrong number).  All arithmetic is
 * 64-bit and exact; a partial sum of one group has one owner on the device and is added once with a 64-bit integer add, so
 * results are reproducible.  GAT_DISTANCE_LDS_PIECES (context option): how many intervals of a searched list the kernel's
 * search finds in LDS before it goes to global memory; it changes no result.
 *
 * gat_list_distances: caller-provided lists.  lists: n_lists * n_groups segment lists (HOST, CSR via list_off, n_lists *
 * n_groups + 1 entries), list l of group g at index l * n_groups + g; annos / anno_off: n_tracks * n_groups annotation lists
 * (HOST, CSR, n_tracks * n_groups + 1 entries), track t of group g at index t * n_groups + g -- the layout of gat_list_metrics
 * and gat_count_lists; max_distance in [0, 2^32]; out_host: [n_lists][n_tracks][4].  Synchronous.  GAT_ERR_ARG: a NULL ctx /
 * list_off / anno_off / out_host (lists / annos may be NULL where they hold nothing), negative counts, a decreasing offset, a
 * direction other than the two, max_distance outside its range, a searched list (the tracks' in direction 0, the segment
 * lists' in direction 1) that is not normalized or holds an empty interval: gat_last_error names the track (or list) and the
 * group. */
#define GAT_DISTANCE_WORDS 4
#define GAT_DISTANCE_SEGMENT_TO_ANNOTATION 0
#define GAT_DISTANCE_ANNOTATION_TO_SEGMENT 1
int gat_list_distances(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                       const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int32_t n_groups,
                       int direction, int64_t max_distance, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_distance behind every batch that passed its checks, reading
 * the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed and
 * range (per-unit streams only).  The groups are the problem's contigs in the problem's order: anno_off has n_tracks *
 * n_contigs + 1 entries; out_host: [sample][track][4], sample_end - sample_begin samples.  Synchronous, like gat_sample.
 * Results do not depend on how the range is cut into batches or calls.  GAT_ERR_ARG: a NULL ctx / p / anno_off / out_host,
 * sample_end < sample_begin, a negative n_tracks, a decreasing anno_off, a direction other than the two, max_distance outside
 * [0, 2^32], in direction 0 a track that is not normalized (gat_last_error names the track and the contig), in direction 1 a
 * sampler whose lists are not normalized (SamplerSegments on a problem without isochore keys; the message says so), a call
 * in flight on the problem.  An empty sample range writes nothing.  The sampler's errors pass through (GAT_ERR_ASSERT;
 * SamplerBruteForce's GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_distances(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                         int64_t sample_begin, int64_t sample_end,
                         const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                         int direction, int64_t max_distance,
                         int64_t* out_host, gat_stats* stats /* nullable */);

/* What a quantitative track -- conservation, GC content, a ChIP or ATAC signal, a methylation level -- amounts to over the
 * segments of a list, formed on the device by k_signal (the reference has nothing like it: its annotations are interval sets).
 * The groups are contigs.  A signal track t on group g is a list of K >= 0 pieces (s_k, e_k, q_k): the intervals normalized --
 * sorted by start, pairwise disjoint, every e_k > s_k; adjacent pieces allowed -- and q_k a SIGNED 32-bit integer with
 * |q_k| <= 2^31 - 1 (INT32_MIN is refused).  The caller quantises; the device never sees a float.  For a segment q = [s, e)
 * with e > s:
 *     c(q, t) = sum_k |[s, e) n [s_k, e_k)|            bases of q that carry a value
 *     w(q, t) = sum_k q_k * |[s, e) n [s_k, e_k)|      signed
 * A (segment list, track) pair gets four int64 words (GAT_SIGNAL_WORDS), summed over the groups and the list's segments, in
 * this order:
 *     n        segments with e > s; the same for every track
 *     covered  sum of c(q, t)
 *     hit      segments with c(q, t) > 0
 *     sum      sum of w(q, t), signed
 * Segments with e <= s are skipped.  The segment lists need be neither sorted nor disjoint (SamplerSegments without isochore
 * keys returns neither): every segment counts on its own.  All arithmetic is integer and exact; a partial sum has one owner on
 * the device and is added once with a 64-bit integer add, so results do not depend on batches, workgroups, the LDS limit or how
 * a range is cut into calls.  GAT_SIGNAL_LDS_PIECES (context option): how many piece ends of a (track, group) the kernel's
 * searches find in LDS before they go to global memory; it changes no result.
 *
 * Never a wrong number: with M[t][g] = sum_k |q_k| * (e_k - s_k), formed in 128 bits on the host, a call is refused
 * (GAT_ERR_ARG; gat_last_error names the track) where it cannot show that every |sum| stays below 2^63.  The bound checked:
 *   - normalized segment lists -- the sampled lists of every problem but SamplerSegments without isochore keys, and a caller's
 *     lists that the host finds normalized: a base counts once, so sum_g M[t][g] < 2^63;
 *   - any other lists: sum_g n_g * M[t][g] < 2^63 -- in gat_list_signal n_g is the most segments one of the call's lists that
 *     are not normalized has on group g; in gat_sample_signal what the contig's region of the sampler's slab holds (where the
 *     slab has to grow in mid-call the bound is checked again before the batch that needed it is reduced; the samples of
 *     earlier batches are then written).
 *
 * gat_list_signal: caller-provided lists.  lists / list_off / n_lists / n_groups: as in gat_list_distances.  pieces / piece_off:
 * n_tracks * n_groups piece lists (HOST, CSR, n_tracks * n_groups + 1 entries), track t of group g at index t * n_groups + g;
 * values: parallel to pieces.  out_host: [n_lists][n_tracks][4].  Synchronous.  GAT_ERR_ARG, with nothing written: a NULL ctx /
 * list_off / piece_off / out_host, a NULL pieces / values / lists where they would hold something, negative counts, a
 * decreasing offset, a track that is not normalized (gat_last_error names the track, the group and the interval), a value of
 * INT32_MIN, the bound above.  n_lists == 0 or n_tracks == 0 writes nothing; n_groups == 0 writes zeros. */
#define GAT_SIGNAL_WORDS 4
int gat_list_signal(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                    const gat_segment* pieces, const int32_t* values, const int64_t* piece_off,
                    int32_t n_tracks, int32_t n_groups, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_signal behind every batch that passed its checks, reading
 * the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed and range
 * (per-unit streams only).  The groups are the problem's contigs in the problem's order: piece_off has n_tracks * n_contigs + 1
 * entries; out_host: [sample][track][4], sample_end - sample_begin samples.  Synchronous, like gat_sample.  GAT_ERR_ARG: a NULL
 * ctx / p / piece_off / out_host, a NULL pieces / values where they would hold something, sample_end < sample_begin, a negative
 * n_tracks, a decreasing piece_off, a track that is not normalized, a value of INT32_MIN, the bound above, a call in flight on
 * the problem.  An empty sample range or n_tracks == 0 writes nothing.  The sampler's errors pass through (GAT_ERR_ASSERT;
 * SamplerBruteForce's GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_signal(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                      int64_t sample_begin, int64_t sample_end,
                      const gat_segment* pieces, const int32_t* values, const int64_t* piece_off,
                      int32_t n_tracks, int64_t* out_host, gat_stats* stats /* nullable */);

/* Where along the genome a segment list overlaps an annotation track, per bin, formed on the device by k_local (the reference
 * has nothing like it: gat-run gives one number per annotation over the whole workspace).  Bin b of group (contig) c is
 * [b * bin_size, (b + 1) * bin_size), b < n_bins[c] = bin_off[c + 1] - bin_off[c] -- the layout of gat_sample_coverage:
 * bin_size in [1, 2^31], bin_off with n_groups + 1 non-decreasing entries.  For a normalized segment list L and a normalized
 * annotation list A of the same group (sorted by start, pairwise disjoint, every interval with end > start; adjacent
 * intervals allowed)
 *     v(L, A, b) = |L n A n bin b|        bases; 0 <= v <= bin_size
 * Overlap at or beyond n_bins[c] * bin_size is not counted.  Over a range of S samples and against an observed value
 * obs[t][bin] >= 0 given by the caller, every (track t, bin) gets five int64 words (GAT_LOCAL_WORDS), in this order:
 *     n_pos    samples with v > 0
 *     sum      of v
 *     sumsq    of v * v   (below 2^64, to be read as unsigned where it passes 2^63)
 *     n_less   samples with v < obs   (all S samples count here and in n_eq, those with v == 0 too)
 *     n_eq     samples with v == obs
 * All arithmetic is 64-bit and exact.  Every word is additive over the samples: a partial sum has one owner on the device and
 * is added once with a 64-bit integer add, so results are reproducible and do not depend on how the range is cut into
 * batches, workgroups or calls -- the words of calls over [0, k) and [k, S) add up to those of the call over [0, S).
 * Context options, none of which changes a result: GAT_LOCAL_WINDOW_BINS -- the bins of a workgroup's window in LDS (clamped
 * to what a workgroup's LDS holds); GAT_LOCAL_SAMPLES_PER_BLOCK -- the run of lists a workgroup takes (default: by the
 * launch); GAT_LOCAL_LDS_PIECES -- how many annotation intervals of a window the kernel's search finds in LDS before it goes
 * to global memory.
 *
 * gat_list_bin_overlaps: the raw v of caller-provided lists (the observed values of the input segments with n_lists == 1).
 * lists / list_off, annos / anno_off, n_tracks, n_groups: as in gat_list_distances.  out_host: [n_lists][n_tracks]
 * [bin_off[n_groups]].  Synchronous.  GAT_ERR_ARG: a NULL ctx / list_off / anno_off / bin_off / out_host (lists / annos may
 * be NULL where they hold nothing), negative counts, a decreasing offset, bin_size outside [1, 2^31], bin_off[0] < 0 or a
 * decreasing bin_off, a segment list or a track that is not normalized or holds an empty interval: gat_last_error names the
 * list (or track) and the group.  Never a wrong number. */
#define GAT_LOCAL_WORDS 5
int gat_list_bin_overlaps(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                          const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int32_t n_groups,
                          int64_t bin_size, const int64_t* bin_off, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_local behind every batch that passed its checks, reading
 * the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed and
 * range (per-unit streams only).  The groups are the problem's contigs in the problem's order: anno_off has n_tracks *
 * n_contigs + 1 entries, bin_off n_contigs + 1; obs_host: [n_tracks][total_bins], total_bins = bin_off[n_contigs];
 * out_host: [n_tracks][total_bins][5].  Synchronous, like gat_sample.  An empty sample range writes zeros.  GAT_ERR_ARG: a
 * NULL ctx / p / anno_off / bin_off / obs_host / out_host, sample_end < sample_begin, a negative n_tracks, a decreasing
 * anno_off, bin_size outside [1, 2^31], bin_off[0] < 0 or a decreasing bin_off, a negative obs, bin_size^2 * samples >= 2^64
 * (sumsq would not fit), a track that is not normalized (gat_last_error names the track and the contig), a sampler whose
 * lists are not normalized (SamplerSegments on a problem without isochore keys; the message says so), a call in flight on
 * the problem.  The sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's GAT_ERR_VALUE "sampling did not
 * converge"). */
int gat_sample_bin_enrichment(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                              int64_t sample_begin, int64_t sample_end,
                              const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                              int64_t bin_size, const int64_t* bin_off, const int64_t* obs_host,
                              int64_t* out_host, gat_stats* stats /* nullable */);

/* Which annotation tracks the segments hit TOGETHER, counted on the device by k_pairs (the reference has nothing like it: a
 * user intersects tracks pairwise and runs one job per pair).  The groups are contigs.  A_t is track t, normalized per group
 * (sorted by start, pairwise disjoint, every interval with end > start; adjacent intervals allowed); q = [s, e), e > s, is a
 * segment of group g:
 *     hit(q, t) = 1  iff  q shares a base with an interval of A_t on g
 *               iff  j < K and A_t[j].start < e,  j = the first index with A_t[j].end > s
 * -- bookended is no hit, one shared base is one, a segment over several intervals of one track hits once.  For a segment
 * list L (all its groups) and tracks i <= j
 *     c(L, i, j) = the segments q of L (e > s) with hit(q, i) and hit(q, j)
 * The segment lists need be neither sorted nor disjoint: every segment counts on its own; segments with e <= s are skipped.
 * For a normalized L, c(L, t, t) is CounterSegmentOverlap (intersectionWithSegments, mode "base").  The P = T (T + 1) / 2 pairs
 * of T tracks are ordered (0,0), (0,1), .., (0,T-1), (1,1), ..:  k(i, j) = i * T - i (i - 1) / 2 + (j - i).
 * Over a range of S samples and against an observed value obs[k] >= 0 given by the caller, every pair gets five int64 words
 * (GAT_PAIR_WORDS) -- those of GAT_LOCAL_WORDS, in the same order and with the same meaning, of c in place of v: n_pos, sum,
 * sumsq (unsigned where it passes 2^63), n_less, n_eq; all S samples count in n_less / n_eq, those with c == 0 too.  All
 * arithmetic is 64-bit and exact.  Every word is additive over the samples: a partial sum has one owner on the device and is
 * added once with a 64-bit integer add, so results do not depend on batches, workgroups, the tile, the run, or how the range is
 * cut into calls -- the words of calls over [0, k) and [k, S) add up to those of the call over [0, S).
 * Context options, none of which changes a result: GAT_PAIRS_LDS_PIECES -- how many interval ends of a (track, group) the
 * kernel's search finds in LDS before it goes to global memory (clamped to what fits beside the counts; 0: none);
 * GAT_PAIRS_SAMPLES_PER_BLOCK -- the run of lists a workgroup takes (default: by the launch).
 *
 * gat_list_pair_hits: the raw c of caller-provided lists (the observed values of the input segments with n_lists == 1).
 * lists / list_off, annos / anno_off, n_tracks, n_groups: as in gat_list_distances.  out_host: [n_lists][P].  Synchronous.
 * n_tracks == 0 or n_lists == 0 writes nothing.  GAT_ERR_ARG: a NULL ctx / list_off / anno_off / out_host (lists / annos may
 * be NULL where they hold nothing), negative counts, n_tracks above GAT_PAIR_MAX_TRACKS (2.1 M pairs, 84 MB of words: a
 * contract number), a decreasing offset, a track that is not normalized or holds an empty interval: gat_last_error names the
 * track and the group.  GAT_ERR_CAPACITY: a list of more than 2^31 - 1 segments.  Never a wrong number. */
#define GAT_PAIR_WORDS 5
#define GAT_PAIR_MAX_TRACKS 2048
int gat_list_pair_hits(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                       const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int32_t n_groups,
                       int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_pairs behind every batch that passed its checks, reading
 * the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed and
 * range (per-unit streams only), for every sampler, SamplerSegments without isochore keys included.  The groups are the
 * problem's contigs in the problem's order: anno_off has n_tracks * n_contigs + 1 entries; obs_host: [P]; out_host: [P][5].
 * Synchronous, like gat_sample.  An empty sample range writes zeros; n_tracks == 0 writes nothing.  GAT_ERR_ARG: a NULL ctx /
 * p / anno_off, a NULL obs_host / out_host with n_tracks > 0, sample_end < sample_begin, a negative n_tracks or one above
 * GAT_PAIR_MAX_TRACKS, a decreasing anno_off, a negative obs, n_max^2 * samples >= 2^64 with n_max the most segments one
 * sample can hold (sumsq would not fit), a track that is not normalized (gat_last_error names the track and the contig), a
 * call in flight on the problem.  The sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's GAT_ERR_VALUE
 * "sampling did not converge"). */
int gat_sample_pair_enrichment(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                               int64_t sample_begin, int64_t sample_end,
                               const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                               const int64_t* obs_host, int64_t* out_host, gat_stats* stats /* nullable */);

/* Gene-set enrichment against the sampled null, counted on the device by k_geneset_hits and k_geneset_terms (the reference's
 * gat-geneset.py tests with a hypergeometric draw, which takes every gene to be hit equally often).
 * GENES.  G genes, 0 .. G-1; gene g owns a set of intervals on the groups (contigs); genes may overlap, nest or coincide.  The
 * host flattens a group's genes into PIECES: the elementary intervals between consecutive gene boundaries that at least one
 * gene covers -- normalized (sorted, pairwise disjoint, end > start; adjacent pieces allowed).  Piece j carries members(j),
 * the ascending, duplicate-free ids of the genes that cover it: a CSR (member_off, members) over the pieces of all groups in
 * the groups' order.  For q = [s, e), e > s, a segment of group g:
 *     hit(q, g') iff q shares a base with a piece that has g' among its members
 *                = g' in members(j0 .. j1 - 1),  j0 = the first piece with end > s,  j1 = the first piece with start >= e
 * -- bookended is no hit, one shared base is one.
 *     H(L)    = the genes hit by any segment of list L, over all its groups: a gene hit by three segments, through four
 *               pieces or on two contigs is in H once
 *     c(L, t) = |H(L) n M_t|,  M_t the genes of term t: a CSR (term_off, term_genes) of ascending, duplicate-free gene ids; a
 *               term may be empty
 * The segment lists need be neither sorted nor disjoint (every sampler, SamplerSegments without isochore keys included);
 * segments with e <= s are skipped.  Over a range of S samples and against an observed value obs[t] >= 0 given by the caller,
 * every term gets five int64 words (GAT_GENESET_WORDS) -- those of GAT_LOCAL_WORDS, in the same order and with the same
 * meaning, of c in place of v: n_pos, sum, sumsq, n_less, n_eq; all S samples count in n_less / n_eq, those with c == 0 too.
 * All arithmetic is 64-bit integer and exact.  A partial sum has one owner on the device and is added once, so the words do
 * not depend on batches, workgroups, tiles, runs or knobs, and the words of calls over [0, k) and [k, S) add up to those of
 * the call over [0, S).  Context options, none of which changes a result: GAT_GENESET_LDS_PIECES -- piece ends of a group the
 * searches find in LDS before they go to global memory (clamped to 32 KB over all groups; 0: none);
 * GAT_GENESET_SAMPLES_PER_BLOCK -- the run of lists a workgroup of either kernel takes (default: by the launch);
 * GAT_GENESET_TERM_TILE -- the terms a workgroup of k_geneset_terms owns (1 .. 256).  GAT_GENESET_MAX_GENES is a contract
 * number: 262 144 bits are a bitmap of 32 KB per list, which leaves half of a 64 KB workgroup for the searches' first level
 * and holds every GENCODE gene and transcript set.
 *
 * gat_list_geneset_hits: the raw c of caller-provided lists (the observed values of the input segments with n_lists == 1).
 * lists / list_off, n_groups: as in gat_list_pair_hits.  pieces / piece_off[n_groups + 1]; member_off[n_pieces + 1], n_pieces
 * = piece_off[n_groups] - piece_off[0], indexed by piece from piece_off[0]; term_off[n_terms + 1].  out_host:
 * [n_lists][n_terms].  Synchronous.  n_terms == 0 or n_lists == 0 writes nothing.  GAT_ERR_ARG, nothing written: a NULL ctx /
 * list_off / piece_off / member_off / term_off / out_host (lists / pieces / members / term_genes may be NULL where they hold
 * nothing), negative counts, a decreasing offset array, pieces that are not normalized (gat_last_error names the group and
 * the piece), a piece with no member, members or term genes outside [0, n_genes) or not strictly ascending (it names the
 * piece or the term), n_genes above GAT_GENESET_MAX_GENES.  Never a wrong number. */
#define GAT_GENESET_WORDS 5
#define GAT_GENESET_MAX_GENES 262144
int gat_list_geneset_hits(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                          const gat_segment* pieces, const int64_t* piece_off, const int64_t* member_off, const int32_t* members,
                          int32_t n_genes, const int64_t* term_off, const int32_t* term_genes, int32_t n_terms,
                          int32_t n_groups, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, the two kernels behind every batch that passed its checks,
 * reading the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed
 * and range (per-unit streams only), for every sampler.  The groups are the problem's contigs in the problem's order:
 * piece_off has n_contigs + 1 entries; obs_host: [n_terms]; out_host: [n_terms][5].  Synchronous, like gat_sample.  An empty
 * sample range writes zeros; n_terms == 0 writes nothing.  GAT_ERR_ARG, nothing written: as above, and a NULL p, a NULL
 * obs_host / out_host with n_terms > 0, sample_end < sample_begin, a negative obs, n_genes^2 * samples >= 2^64 (sumsq would
 * not fit), a call in flight on the problem.  The sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's
 * GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_geneset_enrichment(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                                  int64_t sample_begin, int64_t sample_end,
                                  const gat_segment* pieces, const int64_t* piece_off, const int64_t* member_off,
                                  const int32_t* members, int32_t n_genes, const int64_t* term_off, const int32_t* term_genes,
                                  int32_t n_terms, const int64_t* obs_host, int64_t* out_host, gat_stats* stats /* nullable */);

/* How the segments of a list are distributed around a class of points -- transcription start sites, motif centres, exon ends --
 * formed on the device by k_profile (the reference has nothing like it).  The groups are contigs.  An anchor is (a, sigma): a
 * position a in [0, 2^32 - 1] and a strand sigma in {+1, -1} (anchor_minus 0 / 1).  With w = bin_size in [1, 2^31],
 * H = half_bins in [1, 512], R = H * w <= 2^31 and B = 2 H <= GAT_PROFILE_MAX_BINS offset bins, the offset of base x from the
 * anchor is o = sigma * (x - a) in signed 64-bit arithmetic, x lies in the window iff -R <= o < R, and its bin is
 * floor((o + R) / w): bin b covers the offsets [b * w - R, (b + 1) * w - R).  A plus anchor's window is [a - R, a + R), a minus
 * anchor's (a - R, a + R].  For a normalized segment list L (per group sorted by start, pairwise disjoint, every interval with
 * end > start; adjacent intervals allowed) and the anchors A_{t,g} of track t on group g
 *     GAT_PROFILE_BASES      v(L, t, b) = sum over g, over (a, sigma) in A_{t,g}, over q = [s, e) in L_g of
 *                                         #{ x in [s, e) : bin(x; a, sigma) = b }
 *     GAT_PROFILE_MIDPOINTS  the same with q replaced by [m, m + 1), m = s + (e - s) / 2 in integer division
 * A base counts once per anchor whose window holds it: overlapping windows count with multiplicity.  v sums over all groups:
 * a cell is (track, bin).  With K_t the anchors of track t over all groups, 0 <= v <= K_t * w.  Example (w = 10, H = 2), the
 * segment [85, 112): anchor (100, +) gives v = 5, 10, 10, 2; anchor (100, -) gives 1, 10, 10, 6; the midpoint 98 lands in bin
 * 1 of the plus anchor and in bin 2 of the minus one.
 * anchor_off has n_tracks * n_groups + 1 non-decreasing entries, track t of group g at index t * n_groups + g; within a
 * (track, group) the anchors ascend by position, plus before minus at one position, no (position, strand) twice.
 * Over a range of S samples and against an observed value obs[t][b] >= 0 given by the caller, every (track, bin) gets five
 * int64 words (GAT_PROFILE_WORDS) -- those of GAT_LOCAL_WORDS, in the same order and with the same meaning: n_pos, sum, sumsq
 * (unsigned where it passes 2^63), n_less, n_eq; all S samples count in n_less / n_eq, those with v == 0 too.  All arithmetic
 * is integer and exact.  Every word is additive over the samples: a partial sum has one owner on the device and is added once
 * with a 64-bit integer add, so results do not depend on batches, workgroups, the run, or how the range is cut into calls --
 * the words of calls over [0, k) and [k, S) add up to those of the call over [0, S).  Context options, none of which changes a
 * result: GAT_PROFILE_LDS_ANCHORS -- how many anchor positions of a (track, group) the kernel's search finds in LDS before it
 * goes to global memory (clamped to what a workgroup's LDS holds beside the bins; 0: none);
 * GAT_PROFILE_SAMPLES_PER_BLOCK -- the run of lists a workgroup takes (default: by the launch).
 *
 * gat_list_profile: the raw v of caller-provided lists (the observed values of the input segments with n_lists == 1).
 * lists / list_off, n_groups: as in gat_list_distances.  out_host: [n_lists][n_tracks][B].  Synchronous.  n_lists == 0 or
 * n_tracks == 0 writes nothing.  GAT_ERR_ARG, nothing written: a NULL ctx / list_off / anchor_off / out_host (lists /
 * anchor_pos / anchor_minus may be NULL where they hold nothing), negative counts, a decreasing offset, bin_size, half_bins,
 * half_bins * bin_size or mode out of range, K_t * bin_size >= 2^32 for some track (a value is a 32-bit word on the device),
 * anchors that are out of order, a repeated (position, strand), an anchor_minus other than 0 or 1 (gat_last_error names the
 * track and the group), a segment list that is not normalized (it names the list and the group).  Never a wrong number. */
#define GAT_PROFILE_WORDS 5
#define GAT_PROFILE_MAX_BINS 1024
#define GAT_PROFILE_BASES 0
#define GAT_PROFILE_MIDPOINTS 1
int gat_list_profile(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                     const uint32_t* anchor_pos, const uint8_t* anchor_minus, const int64_t* anchor_off,
                     int32_t n_tracks, int32_t n_groups, int64_t bin_size, int32_t half_bins, int mode,
                     int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_profile behind every batch that passed its checks,
 * reading the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed
 * and range (per-unit streams only).  The groups are the problem's contigs in the problem's order: anchor_off has n_tracks *
 * n_contigs + 1 entries; obs_host: [n_tracks][B]; out_host: [n_tracks][B][5].  Synchronous, like gat_sample.  An empty sample
 * range writes zeros; n_tracks == 0 writes nothing.  GAT_ERR_ARG, nothing written: as above, and a NULL p, a NULL obs_host /
 * out_host with n_tracks > 0, sample_end < sample_begin, a negative obs, (K_t * bin_size)^2 * samples >= 2^64 for some track
 * (sumsq would not fit), a sampler whose lists are not normalized (SamplerSegments on a problem without isochore keys; the
 * message says so), a call in flight on the problem.  The sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's
 * GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_profile_enrichment(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                                  int64_t sample_begin, int64_t sample_end,
                                  const uint32_t* anchor_pos, const uint8_t* anchor_minus, const int64_t* anchor_off,
                                  int32_t n_tracks, int64_t bin_size, int32_t half_bins, int mode,
                                  const int64_t* obs_host, int64_t* out_host, gat_stats* stats /* nullable */);

/* Where the segments of a list sit between the two points that flank them, as a fraction of the gap -- the relative distance
 * test (bedtools reldist, GenometriCorr) -- formed on the device by k_reldist (the reference has nothing like it).  If segments
 * and points ignore each other the fraction is spread evenly over [0, 0.5]; mass near 0 is attraction, near 0.5 avoidance.  The
 * groups are contigs.  The reference points of track t on group g are K >= 0 positions p_0 < p_1 < ... < p_{K-1} in
 * [0, 2^32 - 1], strictly ascending.  A segment q = [s, e), e > s, stands for m = s + (e - s) / 2 in integer division.  With j
 * the first index with p_j > m (K: none), q is INSIDE iff 1 <= j <= K - 1, that is p_{j-1} <= m < p_j, and OUTSIDE otherwise
 * (m < p_0, m >= p_{K-1}, K < 2).  For an inside segment d = min(m - p_{j-1}, p_j - m), gap = p_j - p_{j-1} >= 1 and
 *     bin(q) = min(B - 1, floor(2 * d * B / gap)),      B = n_bins in [1, GAT_RELDIST_MAX_BINS]:
 * bin b covers the relative distances [b / 2B, (b + 1) / 2B), and a relative distance of exactly 0.5 goes to the last bin.
 * Everything is unsigned 64-bit (2 * d * B < 2^43); m <= 2^32 - 2, so m + 1 fits 32 bits and j is the first position >= m + 1.
 * Segments with e <= s are skipped.  The lists need be neither sorted nor disjoint -- every segment counts on its own --, so
 * SamplerSegments without isochore keys is accepted, as in gat_list_distances.  A list has at most 2^31 - 1 segments over all
 * its groups.  Example (points 100, 200; B = 10): [138, 143) has m = 140, d = 40, bin 8; [150, 151) has d = 50 and goes to bin
 * 9; [100, 101) has d = 0, bin 0; [200, 201) is outside.
 * A (list L, track t) pair has W = B + GAT_RELDIST_EXTRA values, summed over all groups, in this order:
 *     index b < B   v_b: the inside segments with bin == b
 *     index B       area: with n = sum_b v_b, C_b = v_0 + ... + v_b and D = sum_{b < B} |B * C_b - (b + 1) * n|, 0 where n == 0,
 *                   else floor(D * 1 000 000 / (n * B * B)) -- the area between the list's ECDF over the bins and the uniform
 *                   one in parts per million (GAT_RELDIST_AREA_SCALE), always <= 10^6.  The 64-bit route, which the kernel
 *                   follows: M = n * B * B < 2^51, D <= M, r = D * 1000, area = (r / M) * 1000 + ((r % M) * 1000) / M --
 *                   exact, and no product passes 2^61
 *     index B + 1   inside: n
 *     index B + 2   outside
 * point_off has n_tracks * n_groups + 1 non-decreasing entries, track t of group g at index t * n_groups + g.
 * Over a range of S samples and against an observed value obs[t][k] >= 0 given by the caller, every (track, value index) gets
 * five int64 words (GAT_RELDIST_WORDS) -- those of GAT_PROFILE_WORDS, in the same order and with the same meaning: n_pos, sum,
 * sumsq (unsigned where it passes 2^63), n_less, n_eq; all S samples count in n_less / n_eq, those with a value of 0 too.  All
 * arithmetic is integer and exact.  Every word is additive over the samples: the words of calls over [0, k) and [k, S) add up
 * to those of the call over [0, S), and results do not depend on batches, workgroups, knobs or the run.  Context options, none
 * of which changes a result: GAT_RELDIST_LDS_POINTS -- how many positions of a (track, group) the kernel's search finds in LDS
 * before it goes to global memory (clamped to what a workgroup's LDS holds beside the bins; 0: none);
 * GAT_RELDIST_SAMPLES_PER_BLOCK -- the run of lists a workgroup takes (default: by the launch).
 *
 * gat_list_reldist: the raw values of caller-provided lists (the observed values of the input segments with n_lists == 1).
 * lists / list_off, n_groups: as in gat_list_distances.  out_host: [n_lists][n_tracks][W].  Synchronous.  n_lists == 0 or
 * n_tracks == 0 writes nothing.  GAT_ERR_ARG, nothing written: a NULL ctx / list_off / point_off / out_host (lists / point_pos
 * may be NULL where they hold nothing), negative counts, a decreasing offset, n_bins outside [1, 1024], positions of a (track,
 * group) that are not strictly ascending (gat_last_error names the track and the group), a list of more than 2^31 - 1
 * segments.  Never a wrong number. */
#define GAT_RELDIST_WORDS 5
#define GAT_RELDIST_MAX_BINS 1024
#define GAT_RELDIST_EXTRA 3
#define GAT_RELDIST_AREA_SCALE 1000000
int gat_list_reldist(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                     const uint32_t* point_pos, const int64_t* point_off, int32_t n_tracks, int32_t n_groups,
                     int32_t n_bins, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_reldist behind every batch that passed its checks,
 * reading the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed
 * and range (per-unit streams only), for every sampler.  The groups are the problem's contigs in the problem's order:
 * point_off has n_tracks * n_contigs + 1 entries; obs_host: [n_tracks][W]; out_host: [n_tracks][W][5].  Synchronous, like
 * gat_sample.  An empty sample range writes zeros; n_tracks == 0 writes nothing.  GAT_ERR_ARG, nothing written: as above, and
 * a NULL p, a NULL obs_host / out_host with n_tracks > 0, sample_end < sample_begin, a negative obs, bound^2 * samples >= 2^64
 * with bound = max(10^6, the most segments a sample can hold) (sumsq would not fit), a call in flight on the problem.  The
 * sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_reldist_enrichment(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                                  int64_t sample_begin, int64_t sample_end,
                                  const uint32_t* point_pos, const int64_t* point_off, int32_t n_tracks, int32_t n_bins,
                                  const int64_t* obs_host, int64_t* out_host, gat_stats* stats /* nullable */);

/* How the segments of a list are distributed along a class of SCALED features and their flanks -- the metagene, or
 * scaled-region profile (deeptools computeMatrix scale-regions, ngs.plot) -- formed on the device by k_metagene (the reference
 * has nothing like it).  Every feature (gene, enhancer, CpG island) is stretched to the same number of body bins, 5' to 3', with
 * flank bins of a fixed size on both sides.  The groups are contigs.  A feature is (fs, fe, sigma): a span 0 <= fs < fe <=
 * 2^32 - 1 with len = fe - fs, and a strand sigma in {+1, -1} (feat_minus 0 / 1).  With Bb = body_bins >= 1, Bf = flank_bins
 * >= 0, w = flank_bin_size in [1, 2^31] (ignored with Bf == 0, but still to be in range), F = Bf * w <= 2^31 and B = 2 Bf + Bb
 * <= GAT_METAGENE_MAX_BINS bins, the window of a feature is the bases [fs - F, fe + F) in signed 64-bit arithmetic (fs - F
 * goes below 0 and fe + F passes 2^32).  For a base x of the window of a PLUS feature
 *     upstream    x < fs          bin = floor((x - (fs - F)) / w)                   in [0, Bf)
 *     body        fs <= x < fe    bin = Bf + floor((x - fs) * Bb / len)             (the product stays below 2^42)
 *     downstream  x >= fe         bin = Bf + Bb + floor((x - fe) / w)
 * and a MINUS feature is the mirror: bin(x; fs, fe, -) = bin(fs + fe - 1 - x; fs, fe, +).  The mirror maps the window onto
 * itself: there is no one-base shift as in the minus window of gat_list_profile.  Body bin k holds the oriented body offsets
 * [ceil(k * len / Bb), ceil((k + 1) * len / Bb)); a feature with len < Bb leaves some body bins without a base, which is
 * defined behaviour.  For a normalized segment list L (per group sorted by start, pairwise disjoint, every interval with
 * end > start; adjacent intervals allowed) and the features of track t on group g
 *     GAT_METAGENE_BASES      v(L, t, b) = sum over g, over the features f of (t, g), over q = [s, e) in L_g of
 *                                          #{ x in [s, e) : x in window(f), bin(x; f) = b }
 *     GAT_METAGENE_MIDPOINTS  the same with q replaced by [m, m + 1), m = s + (e - s) / 2 in integer division
 * A base counts once per feature whose window holds it: overlapping and nested features each get it, as an aggregate plot
 * does.  v sums over all groups: a cell is (track, bin).  With K_t the features of track t over all groups, a flank cell is at
 * most K_t * w, a body cell at most sum_f ceil(len_f / Bb), and most_t is the larger of the two (the flank term only with
 * Bf > 0).  Example (Bb = 4, Bf = 1, w = 10), the feature [100, 110) -- body bins of 3, 2, 3, 2 bases: [100, 103), [103, 105),
 * [105, 108), [108, 110) -- and the segment [95, 112): a plus feature gives v = 5, 3, 2, 3, 2, 2; a minus one gives
 * 2, 3, 2, 3, 2, 5; the midpoint 103 lands in bin 2 of the plus feature and in bin 3 of the minus one.
 * feat_off has n_tracks * n_groups + 1 non-decreasing entries, track t of group g at index t * n_groups + g; within a (track,
 * group) the features ascend by (fs, fe, minus), no (fs, fe, minus) twice; they may overlap and nest.
 * Over a range of S samples and against an observed value obs[t][b] >= 0 given by the caller, every (track, bin) gets five
 * int64 words (GAT_METAGENE_WORDS) -- those of GAT_PROFILE_WORDS, in the same order and with the same meaning: n_pos, sum,
 * sumsq (unsigned where it passes 2^63), n_less, n_eq; all S samples count in n_less / n_eq, those with v == 0 too.  All
 * arithmetic is integer and exact.  Every word is additive over the samples: the words of calls over [0, k) and [k, S) add up
 * to those of the call over [0, S), and results do not depend on batches, workgroups, knobs or the run.  Context options, none
 * of which changes a result: GAT_METAGENE_LDS_FEATURES -- how many entries of the prefix maximum of the ends of a (track,
 * group) the kernel's search finds in LDS before it goes to global memory (clamped to what a workgroup's LDS holds beside the
 * bins; 0: none); GAT_METAGENE_SAMPLES_PER_BLOCK -- the run of lists a workgroup takes (default: by the launch).
 *
 * gat_list_metagene: the raw v of caller-provided lists (the observed values of the input segments with n_lists == 1).
 * lists / list_off, n_groups: as in gat_list_distances.  out_host: [n_lists][n_tracks][B].  Synchronous.  n_lists == 0 or
 * n_tracks == 0 writes nothing.  GAT_ERR_ARG, nothing written: a NULL ctx / list_off / feat_off / out_host (lists /
 * feat_start / feat_end / feat_minus may be NULL where they hold nothing), negative counts, a decreasing offset,
 * body_bins < 1, flank_bins < 0, B > 1024, flank_bin_size outside [1, 2^31], F > 2^31, a mode that is neither of the two, a
 * feature with fe <= fs (fe > 2^32 - 1 has no representation in the argument's type), a feat_minus other than 0 or 1, features
 * that are out of order or repeated (gat_last_error names the track and the group), most_t >= 2^32 for some track (a value is
 * a 32-bit word on the device), a segment list that is not normalized (it names the list and the group).  Never a wrong
 * number. */
#define GAT_METAGENE_WORDS 5
#define GAT_METAGENE_MAX_BINS 1024
#define GAT_METAGENE_BASES 0
#define GAT_METAGENE_MIDPOINTS 1
int gat_list_metagene(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                      const uint32_t* feat_start, const uint32_t* feat_end, const uint8_t* feat_minus, const int64_t* feat_off,
                      int32_t n_tracks, int32_t n_groups, int32_t body_bins, int32_t flank_bins, int64_t flank_bin_size,
                      int mode, int64_t* out_host);

/* ... of the sampled lists: the batch loop shared with gat_sample, k_metagene behind every batch that passed its checks,
 * reading the contig-level lists where gat_sample copies them out -- exactly the lists gat_sample returns for the same seed
 * and range (per-unit streams only).  The groups are the problem's contigs in the problem's order: feat_off has n_tracks *
 * n_contigs + 1 entries; obs_host: [n_tracks][B]; out_host: [n_tracks][B][5].  Synchronous, like gat_sample.  An empty sample
 * range writes zeros; n_tracks == 0 writes nothing.  GAT_ERR_ARG, nothing written: as above, and a NULL p, a NULL obs_host /
 * out_host with n_tracks > 0, sample_end < sample_begin, a negative obs, most_t^2 * samples >= 2^64 for some track (sumsq
 * would not fit), a sampler whose lists are not normalized (SamplerSegments on a problem without isochore keys; the message
 * says so), a call in flight on the problem.  The sampler's errors pass through (GAT_ERR_ASSERT; SamplerBruteForce's
 * GAT_ERR_VALUE "sampling did not converge"). */
int gat_sample_metagene_enrichment(gat_ctx* ctx, gat_problem* p, uint32_t seed,
                                   int64_t sample_begin, int64_t sample_end,
                                   const uint32_t* feat_start, const uint32_t* feat_end, const uint8_t* feat_minus,
                                   const int64_t* feat_off, int32_t n_tracks, int32_t body_bins, int32_t flank_bins,
                                   int64_t flank_bin_size, int mode,
                                   const int64_t* obs_host, int64_t* out_host, gat_stats* stats /* nullable */);

/* Counters only, on caller-provided lists: replaces Engine.computeCounts
 * (gat/Engine.pyx:2164-2204; observed counts) and counter(segments, annotations, workspace)
 * (gat/Engine.pyx:1417-1472).  lists: n_lists*n_groups segment lists (HOST, CSR via list_off),
 * annotations: n_tracks*n_groups lists (HOST, CSR via anno_off), ws_nseg[n_groups] =
 * len(workspace[group]).  counts_host: [n_counters][n_tracks][n_lists] 8-byte slots. */
int gat_count_lists(gat_ctx* ctx, const int32_t* counter_ids, int n_counters,
                    const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                    const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                    const int64_t* ws_nseg, int32_t n_groups, void* counts_host);

/* The same with the annotation lists given as ranges of one array: list (track t, group g) =
 * annos[anno_begin[t * n_groups + g] .. anno_end[t * n_groups + g]) -- what a host that keeps every dictionary's lists
 * in one array passes without copying them into group order. */
int gat_count_list_ranges(gat_ctx* ctx, const int32_t* counter_ids, int n_counters,
                          const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                          const gat_segment* annos, const int64_t* anno_begin, const int64_t* anno_end, int32_t n_tracks,
                          const int64_t* ws_nseg, int32_t n_groups, void* counts_host);

/* Read-only: the record of the context's last count launch (gat_count_report above).  A gat_count_lists call runs on a
 * stream of its own inside the library; its record is copied to the context it was called on. */
int gat_count_last_launch(const gat_ctx* ctx, gat_count_report* out);

/* Read-only: what the sampler stage planned for the newest batch of the context's last sampling call (gat_sampler_report
 * above). */
int gat_sampler_last_launch(const gat_ctx* ctx, gat_sampler_report* out);

/* Sizes of the intersection of two interval dictionaries, for the overlap_* columns of a result row: replaces
 * `overlap = track_segments.clone(); overlap.intersect(annotation_segments); overlap.counts(), overlap.sum()`
 * (AnnotatorResultExtended.__init__, gat/Engine.pyx:1911-1928; SegmentList.intersect, gat/SegmentList.pyx:1469-1549).
 * Host arithmetic on the INPUTS of a run (one merge-join per pair of lists, on host threads); no sample passes here.
 * a: n_groups normalized lists (CSR a_off); b: n_tracks * n_groups normalized lists as ranges of one array, list
 * (t, g) = b[b_begin[t * n_groups + g] .. b_end[..]).  Per track t: pairs_out[t] = number of overlapping (a, b) segment
 * pairs over all groups (= segments of the intersection), bases_out[t] = their total overlap. */
int gat_intersection_sizes(const gat_segment* a, const int64_t* a_off, int32_t n_groups,
                           const gat_segment* b, const int64_t* b_begin, const int64_t* b_end, int32_t n_tracks,
                           int64_t* pairs_out, int64_t* bases_out);

/* Sum of the segment lengths of every list a[begin[l] .. end[l]): SegmentList.sum() (gat/SegmentList.pyx:1607-1614, a
 * Position -- uint32 -- accumulator per list), for the *_size columns of the result rows (AnnotatorResultExtended,
 * gat/Engine.pyx:1911-1928) of a run over 10^4 lists.  Host arithmetic on the inputs, like gat_intersection_sizes. */
int gat_list_sums(const gat_segment* a, const int64_t* begin, const int64_t* end, int64_t n_lists, int64_t* sums_out);

/* IntervalDictionary.toIsochores (gat/Engine.pyx:2837-2855; what IO.applyIsochores, gat/IO.py:188-293, does to the segments,
 * annotations and workspace of a run) for every list of a collection in one call, on host threads.  list l: list_len[l]
 * segments at address list_ptr[l] (HOST; normalized: sorted, disjoint, none empty) of contig list_contig[l]; the isochore
 * classes' segments in coordinates (contig << 32) + position, sorted by start and disjoint (the classes partition the
 * contigs), cls_label[j] = class of segment j in [0, n_classes).  truncate != 0: a segment is cut at the class boundaries
 * (SegmentList.intersect, gat/SegmentList.pyx:1469-1549), else every class a segment touches receives it whole
 * (SegmentList.filter, :1401-1467).  Result list (l, k) = out[out_off[l * n_classes + k] .. out_off[l * n_classes + k + 1]).
 * Two calls: with out == NULL the lists are counted (out_off[0 .. n_lists * n_classes] filled, total in *n_out), with out
 * and the same out_off they are written.  Returns GAT_OK, GAT_ERR_ARG, or 1 when a list is not normalized (nothing is
 * written: the host then splits list by list and raises what the reference raises).  Input pipeline; no sample passes here. */
int gat_isochore_split(const uint64_t* list_ptr, const int64_t* list_len, const int64_t* list_contig, int64_t n_lists,
                       const int64_t* cls_start, const int64_t* cls_end, const int64_t* cls_label, int64_t n_cls,
                       int32_t n_classes, int32_t truncate, gat_segment* out, int64_t* out_off, int64_t* n_out);

/* ---- the reference's own random stream ---------------------------------------------------
 * scripts/gat-run.py:267-271 seeds numpy's global generator ONCE and every (sample, unit) of the run -- in the order of
 * gat/__init__.py:531-541, segment track after segment track -- draws from that one MT19937.  gat_sample_and_count's
 * per-unit streams are what makes the samples independent work; this entry reproduces an unpatched reference instead,
 * table for table, at the speed of one stream: one wave runs the samples [0, n_samples) one after the other.
 * mt_state: GAT_MT_STATE_WORDS words, the 624 state words + the position (numpy's `pos`, 624 after seeding); read at
 * entry, written back at return, so that calls (batches, segment tracks) continue each other.  gat_mt19937_seed fills
 * it as numpy.random.seed(seed) does for an integer seed.  Counts as in gat_sample_and_count with sample_begin 0. */
#define GAT_MT_STATE_WORDS 625
void gat_mt19937_seed(uint32_t seed, uint32_t* mt_state);
int gat_sample_and_count_serial(gat_ctx* ctx, gat_problem* prob, const int32_t* counter_ids, int n_counters,
                                uint32_t* mt_state, int64_t n_samples, void* counts_dev, gat_stats* stats);

/* ---- null-distribution statistics on the device -----------------------------------------
 * The numbers AnnotatorResult takes from a row of sampled counts (makeEnrichmentStatistics / getTwoSidedPValue,
 * gat/Engine.pyx:1635-1718, :1543-1576), computed from the count matrix where gat_sample_and_count left it:
 * counts_dev = n_rows rows of n_samples 8-byte slots (int64, or IEEE double for rows with is_double != 0 --
 * nucleotide-density).  Per row r, out_host[8r..8r+8) = { numpy.mean, the sum of squared deviations from it as numpy.std
 * forms it (std = sqrt(that / n_samples); bit for bit: numpy's chunked pairwise summation is restated), the values at sorted positions lo_index and hi_index, the number of samples < vals[r], the
 * number == vals[r], 0, 0 }.  The caller turns them into expected / CI / stddev / p-value as the reference does. */
int gat_null_stats(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples,
                   const uint8_t* is_double_host, const double* vals_host, int64_t lo_index, int64_t hi_index,
                   double* out_host);

/* ---- a null distribution deeper than a count matrix: rounds folded into integer words --------
 * gat_null_stats needs the whole null distribution of a row in one matrix.  A run that draws more samples than a matrix
 * holds draws them in rounds into ONE buffer (sample s is the same sample whichever call draws it: the per-unit contract)
 * and folds every round, where gat_sample_and_count left it, into GAT_NULL_FOLD_WORDS uint64 words per row:
 *     n   sum of v   sumsq_lo, sumsq_hi: the sum of v * v modulo 2^128   n_less = #{v < val}   n_eq = #{v == val}   min   max
 * counts_dev: n_rows rows of non-negative int64 (0 <= v < 2^63; not the IEEE rows of nucleotide-density), of which the
 * first n_samples slots are used; rows lie row_stride >= n_samples slots apart (a run's last, short round reuses the
 * buffer).  vals_host[r]: the value the row's p-value will be asked for.  Integer arithmetic only: the host turns val into
 * ceil(val) clamped to [0, 2^63] (for an integer v, v < val is v < ceil(val)) and into the integer v has to equal, none when
 * val is not an integer a slot can hold; v * v is the full 128-bit product, added with its carry; sum is modulo 2^64 (a
 * caller that wants it keeps n * max below that).  words_dev += this round: the words of disjoint sample ranges add, in
 * any order and under any launch shape -- GAT_NULL_FOLD_PARTS (a context option, default 0: by the launch, else 1 .. 1024)
 * is the number of workgroups a row is cut over and changes no word.  gat_null_fold_reset: all words 0, min = 2^64 - 1.
 * Both return after their kernel has completed.  n_rows == 0: GAT_OK, nothing touched.  GAT_ERR_ARG: a NULL argument,
 * n_rows < 0, n_samples < 1, row_stride < n_samples, a val that is NaN or infinite, the option out of range. */
#define GAT_NULL_FOLD_WORDS 8   /* n, sum, sumsq_lo, sumsq_hi, n_less, n_eq, min, max -- uint64 each */
int gat_null_fold_reset(gat_ctx* ctx, uint64_t* words_dev, int64_t n_rows);
int gat_null_fold(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples, int64_t row_stride,
                  const double* vals_host, uint64_t* words_dev);

/* ---- gat-compare: the null distribution of a fold-change difference, and its statistics -------
 * What scripts/gat-compare.py:214-231 of the reference forms for a pair (data1, data2) of result rows read from counts
 * files, and what AnnotatorResult then takes from it, without the row ever existing on the host.  a_dev / b_dev: DEVICE
 * matrices [n_rows_a][n_samples] / [n_rows_b][n_samples] of float64 sampled counts (the same matrix when annotations of one
 * run are compared).  Pair p = rows (ia[p], ib[p]); for every sample i, in this order of IEEE operations,
 *     fc1 = obs_a[p] / (a[ia[p]][i] + pseudo_count) + 0.0001,  fc2 = obs_b[p] / (b[ib[p]][i] + pseudo_count) + 0.0001,
 *     row[i] = log(fc1 / fc2) + delta[p]
 * (the additions and divisions are numpy's bit for bit; the device's log and numpy's each are good to about an ulp and not
 * the same function).  out_host[8p..8p+8) = what gat_null_stats returns for that row with vals = delta[p] -- { mean, sum of
 * squared deviations, the values at sorted positions lo_index and hi_index, samples < delta[p], samples == delta[p] } --
 * then, slot 6, the number of samples of the row that are not finite (a zero denominator: inf, inf / inf: nan, as numpy
 * gives them; the other slots of such a pair are not to be used -- the host recomputes it), and 0.  Pairs are worked on in
 * batches whose rows fit GAT_COMPARE_SCRATCH_MB megabytes of device scratch (a context option, default 1024; read once at
 * the top of the call).  GAT_ERR_ARG: a NULL argument, a row index outside its matrix, bad positions; GAT_ERR_CAPACITY:
 * more samples per row than k_null_stats takes. */
int gat_compare_stats(gat_ctx* ctx, const void* a_dev, int64_t n_rows_a, const void* b_dev, int64_t n_rows_b,
                      int64_t n_samples, const int32_t* ia_host, const int32_t* ib_host, int64_t n_pairs,
                      const double* obs_a_host, const double* obs_b_host, const double* delta_host,
                      double pseudo_count, int64_t lo_index, int64_t hi_index, double* out_host);

/* ---- step-down minP: family-wise adjusted p-values from the joint null distribution --------
 * Westfall and Young's step-down minP procedure (as formulated by Ge, Dudoit and Speed 2003) on a count matrix: column i is
 * what every row of the family scored on the same sample.  counts_dev = n_rows rows of n_samples 8-byte slots, the layout
 * gat_null_stats reads (int64, or IEEE double for rows with is_double != 0; compared as doubles).  With
 *     n_less = #{i : row_r[i] < x},  n_eq = #{i : row_r[i] == x}
 *     T(r, x) = max(1, idx),  idx = 1 if n_less == S,  S - (n_less - [n_eq > 0 and n_less > 0] + 1) if x > means[r],
 *                                   n_less + n_eq otherwise
 * (S = n_samples; T / S is getTwoSidedPValue, gat/Engine.pyx:1543-1576, with expected = means[r]) and kobs[r] = T(r, the
 * row's observed value), formed by the caller:  K[r][i] = T(r, row_r[i]);  the rows ordered by (kobs, r) ascending are
 * o_1 .. o_R;  q_{R+1}[i] = +inf, q_j[i] = min(q_{j+1}[i], K[o_j][i]);  c_out[o_j] = #{i : q_j[i] <= kobs[o_j]}.
 * c_out is in the order of the input rows and BEFORE the running maximum: the adjusted p-value of o_j is the largest of
 * max(1, c_out[o_j']) / S over j' <= j, which the caller forms.  All of it is integer arithmetic.
 * k_minp_rank sorts every row (in LDS up to GAT_MINP_LDS_SAMPLES samples, default 4096, at most what a workgroup's LDS
 * holds; beyond in device scratch) and ranks its samples in it; k_minp_step takes the running minimum through the rows,
 * which are worked on in batches of as many rows of K (4 bytes a sample) as fit GAT_MINP_SCRATCH_MB megabytes (default
 * 1024).  Both are context options read once at the top of the call; neither changes a result.  n_rows <= 0: GAT_OK, nothing
 * written.  GAT_ERR_ARG: a NULL argument, n_samples < 1 or >= 2^31, a kobs outside [1, n_samples], an option out of range. */
int gat_minp_counts(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples,
                    const uint8_t* is_double_host, const double* means_host, const int32_t* kobs_host,
                    int64_t* c_out_host /* n_rows, input row order, before the running maximum */);
/* device time in milliseconds the context's last gat_minp_counts spent in k_minp_rank and in k_minp_step, summed over its
 * batches; measured only after gat_ctx_set_kernel_times(ctx, 1) (or GAT_KERNEL_TIMES), else 0 */
int gat_minp_times(const gat_ctx* ctx, float* ms_rank, float* ms_step);

/* ---- resampling-based FDR: the expected number of false calls from the joint null distribution --------
 * The FDR counterpart of step-down minP, and what the Annotator's "False Discovery summary" estimates: the number of rows of
 * column i that would be called at a threshold is one draw of the number of false calls there.  counts_dev, is_double, means,
 * kobs, T and K[r][i] = T(r, row_r[i]) are those of gat_minp_counts (S = n_samples).  With
 *     D[r][i] = 1 if row_r[i] > means[r] else 0        (the comparison T branches on: 1 = the over-represented tail)
 *     V_d(t)  = #{(r, i) : K[r][i] <= t and D[r][i] == d},  d in {1, 0}
 *     N_d[i]  = #{r : K[r][i] <= L and D[r][i] == d}   for a level L
 * v_out[r] = { V_1(kobs[r]), V_0(kobs[r]) } in the order of the input rows, and per_sample_out[l] = { N_1[0..S), N_0[0..S) }
 * for L = levels[l].  A sample counts as significant at t exactly when an observed value equal to it would.  The caller
 * forms Rn(t) = #{r : kobs[r] <= t}, fdr(t) = (V_1(t) + V_0(t)) / (S * Rn(t)) and, along the rows o_1 .. o_R ordered by
 * (kobs, r) ascending, q[o_j] = min(1, max(1 / S, min over j' >= j of fdr(kobs[o_j']))); and from N the summary per level
 * (mean, median, 95 % limit over the samples).  All of it is integer arithmetic; a level 0 gives zeros (K >= 1).
 * The rows are ranked into K as gat_minp_counts does it (k_minp_rank, batches of GAT_MINP_SCRATCH_MB, GAT_MINP_LDS_SAMPLES,
 * GAT_MINP_ALL_PASSES); k_efdr then makes one pass over a batch's K and the matrix (D is recomputed from it) per chunk of at
 * most GAT_EFDR_LDS_THRESHOLDS distinct kobs (default and upper limit: what a workgroup's LDS holds at 12 bytes a threshold,
 * 13653 with 160 KiB), counting into LDS bins and from there into 64-bit bins on the device, whose prefix sums are V.  All
 * are context options read once at the top of the call; none changes a result.  n_rows <= 0: GAT_OK, nothing written.
 * GAT_ERR_ARG: a NULL argument (levels_host and per_sample_out_host may be NULL when n_levels == 0), n_samples < 1 or
 * >= 2^31, a kobs outside [1, n_samples], n_levels outside [0, 8], a level outside [0, n_samples], an option out of range. */
int gat_efdr_counts(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples,
                    const uint8_t* is_double_host, const double* means_host, const int32_t* kobs_host,
                    const int32_t* levels_host, int32_t n_levels,
                    int64_t* v_out_host          /* [n_rows][2]: V_1(kobs[r]), V_0(kobs[r]), input row order */,
                    int32_t* per_sample_out_host /* [n_levels][2][n_samples]: N_1, N_0; may be NULL when n_levels == 0 */);
/* device time in milliseconds the context's last gat_efdr_counts spent in k_minp_rank and in k_efdr (all its chunks), summed
 * over its batches; measured only after gat_ctx_set_kernel_times(ctx, 1) (or GAT_KERNEL_TIMES), else 0 */
int gat_efdr_times(const gat_ctx* ctx, float* ms_rank, float* ms_efdr);

/* ---- multi-GPU: the one collective of the path ---------------------------------------------
 * Replaces the result collation of the reference's process pool (gat/__init__.py:681-700, :770-774):
 * every rank has computed the columns of its own contiguous sample range (gat_sample_and_count with
 * [sample_begin, sample_end) = its shard) and ONE all-gather over xGMI makes every rank hold all of them.
 * RCCL is loaded at the first call (dlopen of librccl.so: the library has no link-time dependency on it);
 * a host without it gets GAT_ERR_DEVICE.  Ranks are processes, one per GPU; rank 0 calls
 * gat_comm_unique_id and passes the 128 bytes to the others by whatever means the host has (the Python host
 * uses torch.distributed's store or MPI; a file works).  torch.distributed's "nccl" backend is the same
 * RCCL: gat_amd/distributed.py uses it when a process group exists and needs none of this. */
typedef struct gat_comm gat_comm;
#define GAT_COMM_ID_BYTES 128
int gat_comm_unique_id(void* id_out /* GAT_COMM_ID_BYTES */);
int gat_comm_create(gat_ctx* ctx, gat_comm** out, int n_ranks, int rank, const void* id /* GAT_COMM_ID_BYTES */);
void gat_comm_destroy(gat_comm* comm);
/* send_dev: this rank's n_slots 8-byte slots (its [counter][track][shard] block); recv_dev: n_ranks * n_slots
 * slots, rank r's block at r * n_slots.  Enqueued on the ctx stream; returns after completion. */
int gat_allgather_counts(gat_ctx* ctx, gat_comm* comm, const void* send_dev, void* recv_dev, int64_t n_slots);
/* Which RCCL the calls above resolved: 1 = one the process had mapped already (a host with torch holds torch/lib/librccl.so: it
 * is found with RTLD_NOLOAD / among the process's objects and used -- a process never holds two RCCLs), 0 = loaded afresh
 * (librccl.so, librccl.so.1, /opt/rocm/lib/librccl.so, or $GAT_RCCL_LIB), -1 = none found. */
int gat_comm_library_preloaded(void);

/* queries */
int gat_problem_info(const gat_problem* p, int64_t* n_units, int64_t* n_contigs, int64_t* n_tracks,
                     int64_t* slab_segments_per_sample, int64_t* algorithmic_bytes_per_sample);

/* raw MT19937 outputs generated ahead per sample (over all units: the rows of k_rng), to set against gat_stats.n_draws, the
 * outputs the samples consumed */
int64_t gat_problem_rng_rows(const gat_problem* p);

#ifdef __cplusplus
}
#endif
#endif
