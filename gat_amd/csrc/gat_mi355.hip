// gat_mi355.hip -- host side of libgat_mi355.so (C ABI in include/gat_mi355.h).
//
// Host work is limited to what the reference does once per (segments, workspace) pair before
// sampling starts (gat/Engine.pyx:543-565, hoisted out of the per-sample loop), buffer management
// and kernel launches.  Sampling, fromIsochores and counting run only as HIP kernels
// (gat_kernels.h); there is no CPU path for them in this library.
//
// In this file: the context, the scratch, the count launches, the sampler batch and the call seam (gat_sample_and_count*),
// gat_count_lists, the RCCL entry points and the statistics.  gat_list_calls.h, included behind the call seam: gat_sample /
// gat_sample_units and the list reductions (gat_sample_* / gat_list_* of coverage, metrics, distances, signal, gat-local,
// gat-pairs, gat-geneset, gat-profile, gat-reldist and gat-metagene).  One translation unit: the Makefile keeps its device assembly and checks it.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <link.h>            // dl_iterate_phdr: the RCCL a host process has mapped already
#include <rccl/rccl.h>          // types only: the library is loaded with dlopen at the first collective

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <climits>
#include <string>
#include <vector>
#include <thread>
#include <chrono>
#include <atomic>

#include "../../include/gat_mi355.h"
#define GAT_NUM_COUNTERS_DEV 6
#include "gat_kernels.h"
#include "gat_tail.h"
#include "gat_shift.h"
#include "gat_permute.h"
#include "gat_local_permute.h"
#include "gat_circular.h"
#include "gat_universe.h"
#include "gat_brute_force.h"
#include "gat_stats.h"
#include "gat_null_fold.h"
#include "gat_compare.h"
#include "gat_minp.h"
#include "gat_efdr.h"
#include "gat_coverage.h"
#include "gat_metrics.h"
#include "gat_distance.h"
#include "gat_signal.h"
#include "gat_local.h"
#include "gat_pairs.h"
#include "gat_geneset.h"
#include "gat_profile.h"
#include "gat_reldist.h"
#include "gat_metagene.h"


#include "gat_host.h"
#include "gat_metrics_tables.h"

thread_local std::string g_last_error;

// ------------------------------------------------------------------------------------------
extern "C" const char* gat_version(void) { return "gat_mi355 0.1 (gfx950)"; }

extern "C" const char* gat_last_error(const gat_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

extern "C" int gat_ctx_create(gat_ctx** out, int device_id, void* stream) {
  if (!out) return set_err(nullptr, GAT_ERR_ARG, "gat_ctx_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return set_err(nullptr, GAT_ERR_DEVICE, "no HIP device available (%s): this library has no CPU path",
                   e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev) return set_err(nullptr, GAT_ERR_ARG, "device %d out of range (0..%d)", device_id, ndev - 1);
  gat_ctx* ctx = new gat_ctx();
  ctx->device = device_id;
  HIPCHK(ctx, hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIPCHK(ctx, hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    int rc = set_err(nullptr, GAT_ERR_DEVICE, "device %d is %s; this library carries gfx950 code only", device_id, prop.gcnArchName);
    delete ctx;
    return rc;
  }
  ctx->max_lds = (int)prop.sharedMemPerBlock;
  if (ctx->max_lds < 160 * 1024) ctx->max_lds = 160 * 1024;   // gfx950: 160 KiB per workgroup via the opt-in attribute
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  for (auto& ev : ctx->ev) HIPCHK(ctx, hipEventCreate(&ev));
  for (auto& ev : ctx->ev_main) HIPCHK(ctx, hipEventCreate(&ev));
  for (auto& ev : ctx->ev_k) HIPCHK(ctx, hipEventCreate(&ev));
  for (auto& ev : ctx->ev_t) HIPCHK(ctx, hipEventCreate(&ev));
  for (auto& ev : ctx->ev_cnt) HIPCHK(ctx, hipEventCreate(&ev));
  HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_flags, 64, hipHostMallocDefault));
  HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_stat, gat::kStatSlotWords * 8, hipHostMallocDefault));
  memset(ctx->h_stat, 0, gat::kStatSlotWords * 8);
  *out = ctx;
  return GAT_OK;
}

// pinned words + events of a call in flight: taken from the context's idle blocks, made when there is none
static int call_block_get(gat_ctx* ctx, CallBlock** out) {
  if (!ctx->call_blocks.empty()) { *out = ctx->call_blocks.back(); ctx->call_blocks.pop_back(); return GAT_OK; }
  std::unique_ptr<CallBlock> b(new CallBlock());
  static_assert(CallBlock::kStatBytes == (size_t)kMaxInflight * gat::kStatSlotWords * 8, "the slots as allocated and as stat_slot() indexes them");
  HIPCHK(ctx, hipHostMalloc((void**)&b->h_stat, CallBlock::kStatBytes + 512 * 8, hipHostMallocDefault));
  b->h_mstat = b->stat_slot(kMaxInflight);         // (behind the last slot)
  HIPCHK(ctx, hipEventCreate(&b->ev_begin));
  HIPCHK(ctx, hipEventCreate(&b->ev_end));
  for (auto& pair : b->ev_main) for (auto& ev : pair) HIPCHK(ctx, hipEventCreate(&ev));
  HIPCHK(ctx, hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
  HIPCHK(ctx, hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
  *out = b.release();
  return GAT_OK;
}
static void call_block_free(CallBlock* b) {
  if (!b) return;
  if (b->h_stat) (void)hipHostFree(b->h_stat);
  if (b->ev_begin) (void)hipEventDestroy(b->ev_begin);
  if (b->ev_end) (void)hipEventDestroy(b->ev_end);
  for (auto& pair : b->ev_main) for (auto& ev : pair) if (ev) (void)hipEventDestroy(ev);
  if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
  if (b->ev_join) (void)hipEventDestroy(b->ev_join);
  delete b;
}

// the context lives as long as its handle or a problem made on it does (a host may close them in either order)
void ctx_release(gat_ctx* ctx);
extern "C" void gat_ctx_destroy(gat_ctx* ctx) {
  if (!ctx || ctx->closed) return;
  ctx->closed = true;
  ctx_release(ctx);
}
void ctx_release(gat_ctx* ctx) {
  if (--ctx->refs > 0) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& lane : ctx->lanes) if (lane) { (void)hipStreamSynchronize(lane); (void)hipStreamDestroy(lane); lane = nullptr; }
  ctx->stage_used = 0;
  for (CallBlock* b : ctx->call_blocks) call_block_free(b);
  ctx->call_blocks.clear();
  if (ctx->build_ctx) { gat_ctx_destroy(ctx->build_ctx); ctx->build_ctx = nullptr; }
  if (ctx->aux_ctx) { gat_ctx_destroy(ctx->aux_ctx); ctx->aux_ctx = nullptr; }
  for (auto& ev : ctx->ev) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : ctx->ev_main) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : ctx->ev_k) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : ctx->ev_t) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : ctx->ev_cnt) if (ev) (void)hipEventDestroy(ev);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  if (ctx->h_flags) (void)hipHostFree(ctx->h_flags);
  if (ctx->h_stat) (void)hipHostFree(ctx->h_stat);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

extern "C" int gat_ctx_set_kernel_times(gat_ctx* ctx, int on) {
  if (!ctx) return set_err(nullptr, GAT_ERR_ARG, "ctx is NULL");
  ctx->kernel_times = on != 0;
  return GAT_OK;
}

extern "C" int gat_call_lane_for(int n_lanes, int asynchronous, int timed, int serial_state, int others_in_flight, const int32_t* lane_busy) {
  bool busy[kMaxLanes] = {};
  for (int l = 0; l < kMaxLanes && l < n_lanes; ++l) busy[l] = lane_busy != nullptr && lane_busy[l] != 0;
  return call_lane_for(n_lanes, asynchronous != 0, timed != 0, serial_state != 0, others_in_flight, busy);
}

extern "C" void* gat_ctx_stream(const gat_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int gat_ctx_synchronize(gat_ctx* ctx) {
  if (!ctx) return set_err(nullptr, GAT_ERR_ARG, "ctx is NULL");
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return GAT_OK;
}

extern "C" int gat_dev_alloc(gat_ctx* ctx, void** out, size_t bytes) {
  if (!ctx || !out) return set_err(ctx, GAT_ERR_ARG, "gat_dev_alloc: NULL argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (bytes == 0) bytes = 1;
  HIPCHK(ctx, dev_pool_alloc(out, bytes));
  ctx->user_allocs.push_back(std::make_pair(*out, bytes));
  return GAT_OK;
}
extern "C" int gat_dev_free(gat_ctx* ctx, void* p) {
  if (!ctx) return set_err(ctx, GAT_ERR_ARG, "gat_dev_free: NULL ctx");
  if (!p) return GAT_OK;
  for (size_t i = 0; i < ctx->user_allocs.size(); ++i)
    if (ctx->user_allocs[i].first == p) {
      // (the caller may free right behind work it enqueued on the context's stream: a pooled block must be idle)
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      dev_pool_free(p, ctx->user_allocs[i].second);
      ctx->user_allocs.erase(ctx->user_allocs.begin() + (long)i);
      return GAT_OK;
    }
  HIPCHK(ctx, hipFree(p));
  return GAT_OK;
}
extern "C" int gat_memcpy_d2h(gat_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return set_err(ctx, GAT_ERR_ARG, "NULL ctx");
  HIPCHK(ctx, staged_d2h(ctx, dst, src, bytes));
  return GAT_OK;
}
extern "C" int gat_memcpy_h2d(gat_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return set_err(ctx, GAT_ERR_ARG, "NULL ctx");
  HIPCHK(ctx, staged_h2d(ctx, dst, src, bytes));
  return GAT_OK;
}

// ------------------------------------------------------------------------------------------
static int ensure_scratch(gat_ctx* ctx, gat_problem* P, const Knobs& kn, int64_t want) {
  if (P->batch >= want) return GAT_OK;
  PrepTimer tm;
  // a batch as large as a quarter of the 288 GB takes: the lane-per-stream kernels have a fixed floor per launch (the serial
  // chain of the longest unit's tile) and the wave-per-unit kernels of long-list problems fill the chip only with
  // thousands of samples in flight, so fewer, larger batches are faster (config 3, 10 000 samples: 9.7 ms in two batches
  // under 12 GB, 9.3 ms in one; config-4 shape: a rank's shard of 12 500 samples in one batch of 40 GB instead of two);
  // capped by what the device has free
  double budget = kn.slab_bytes;
  if (!kn.slab_bytes_set) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      budget = std::min(std::min(budget, 0.25 * (double)total_b), 0.6 * (double)(free_b + dev_pool_held()));
  }
  const int64_t per_sample = P->slab_stride * 8 * (P->merge_contigs ? 2 : 1) + 4 * ((int64_t)P->n_units + P->n_contigs) +
                             (P->sampler_mode ? P->rng_rows_total * 4 + 16 * (int64_t)P->n_units : 0) +
                             (P->split_path ? P->slab_stride * 8 + P->slab_stride / 2 + (int64_t)(sizeof(gat::TailPatch) + 4) * P->n_units : 0);
  int64_t b = (int64_t)(budget / (double)per_sample);
  b = std::max<int64_t>(1, std::min<int64_t>(b, want));
  if (P->batch >= b) return GAT_OK;
  HIPCHK(ctx, P->d_slab.alloc((size_t)(b * P->slab_stride)));
  if (P->merge_contigs) HIPCHK(ctx, P->d_cslab.alloc((size_t)(b * P->slab_stride)));
  HIPCHK(ctx, P->d_unit_n.alloc((size_t)(b * std::max(1, P->n_units))));
  HIPCHK(ctx, P->d_contig_n.alloc((size_t)(b * std::max(1, P->n_contigs))));
  HIPCHK(ctx, P->d_ws_stat.alloc((size_t)(b * std::max(1, P->n_units)) * 4));
  HIPCHK(ctx, hipMemsetAsync(P->d_unit_n.p, 0, (size_t)(b * std::max(1, P->n_units)) * 4, call_stream(ctx, P)));
  HIPCHK(ctx, hipMemsetAsync(P->d_contig_n.p, 0, (size_t)(b * std::max(1, P->n_contigs)) * 4, call_stream(ctx, P)));
  HIPCHK(ctx, hipMemsetAsync(P->d_ws_stat.p, 0, (size_t)(b * std::max(1, P->n_units)) * 16, call_stream(ctx, P)));
  if (P->sampler_mode) {
    const int64_t nsb = (b + 63) / 64;
    P->h_rng_off.assign(P->h_order.size() + 1, 0);
    for (size_t a = 0; a < P->h_order.size(); ++a) P->h_rng_off[a + 1] = P->h_rng_off[a] + nsb * (int64_t)P->h_rng_rows[a] * 64;
    HIPCHK(ctx, P->d_rng_off.alloc(P->h_rng_off.size()));
    HIPCHK(ctx, staged_h2d(ctx, P->d_rng_off.p, P->h_rng_off.data(), P->h_rng_off.size() * 8));
    HIPCHK(ctx, P->d_rng_out.alloc((size_t)P->h_rng_off.back()));
    HIPCHK(ctx, P->d_rng_ckpt.alloc((size_t)nsb * std::max<size_t>(1, P->h_order.size()) * gat::kRngWaves * gat::kWave));
    const size_t ns = (size_t)(b * std::max(1, P->n_units));
    HIPCHK(ctx, P->d_st.alloc(ns));
    HIPCHK(ctx, P->d_st2.alloc(ns));
    if (!P->split_path && P->long_lists) {                                      // k_tail_big's hand-over records
      HIPCHK(ctx, P->d_patch.alloc(ns));
      HIPCHK(ctx, hipMemsetAsync(P->d_patch.p, 0, ns * sizeof(gat::TailPatch), call_stream(ctx, P)));
      HIPCHK(ctx, P->d_todo.alloc(ns));                                         // ... and the queue of what k_resume_big leaves
    }
    if (P->split_path) {
      HIPCHK(ctx, P->d_cum.alloc((size_t)(b * P->slab_stride / 8 + 8)));      // (slab regions are multiples of 64 entries: cap_for)
      HIPCHK(ctx, P->d_fslab.alloc((size_t)(b * P->slab_stride)));
      HIPCHK(ctx, P->d_patch.alloc(ns));
      HIPCHK(ctx, P->d_todo.alloc(ns));
    }
  }
  P->batch = b;
  tm.lap("scratch for the batch");
  return GAT_OK;
}

struct Counters {
  int32_t slot[GAT_NUM_COUNTERS];
  bool any_seg = false, any_anno = false;
};

static int parse_counters(gat_ctx* ctx, const int32_t* ids, int n, Counters& C) {
  for (int i = 0; i < GAT_NUM_COUNTERS; ++i) C.slot[i] = -1;
  for (int k = 0; k < n; ++k) {
    if (ids[k] < 0 || ids[k] >= GAT_NUM_COUNTERS) return set_err(ctx, GAT_ERR_ARG, "unknown counter id %d", ids[k]);
    if (C.slot[ids[k]] >= 0) return set_err(ctx, GAT_ERR_ARG, "counter id %d given twice", ids[k]);
    C.slot[ids[k]] = k;
    if (ids[k] <= GAT_COUNTER_SEGMENT_MIDOVERLAP) C.any_seg = true; else C.any_anno = true;
  }
  return GAT_OK;
}

static_assert(gat::kMergedThreads / gat::kWave == kMergedWavesHost, "gat_host.h: kMergedWavesHost");
// which kernel serves the segment-side counters (the choice launch_count makes)
// merged_only: the tables were BUILT for that route alone (AnnoDev::per_track false -- decided from the knobs as they were then):
// the route stands whatever the knobs say now (a knob flipped between the build and the call was GAT_ERR_ARG)
static int count_route(const gat_ctx* ctx, const Knobs& kn, bool has_merged, const Counters& C, int n_contigs, int n_tracks, int swap_capx,
                       bool merged_only = false) {
  if (!C.any_seg || n_contigs <= 0) return GAT_COUNT_KERNEL_NONE;
  const bool only_overlap = C.slot[GAT_COUNTER_SEGMENT_OVERLAP] < 0 && C.slot[GAT_COUNTER_SEGMENT_MIDOVERLAP] < 0;
  const size_t lds_merged = (size_t)n_tracks * 4 * (gat::kMergedThreads / gat::kWave);
  if (only_overlap && has_merged && (int64_t)lds_merged + 1024 <= ctx->max_lds && (merged_only || !kn.count_no_merged))
    return GAT_COUNT_KERNEL_MERGED;
  if (swap_capx > 0 && only_overlap && !kn.count_no_swap) return GAT_COUNT_KERNEL_SWAP;
  return GAT_COUNT_KERNEL_SEG;
}

// launch the count kernels over n_lists sample lists
// ev_main: the pair of events recorded around the dominant kernel; main_recorded / count_kernel: what was launched
struct CountLaunch {
  hipStream_t stream = nullptr;  // where the kernels and the events go: the call's (call_stream), the context's (gat_count_lists)
  hipEvent_t* ev_main = nullptr;
  bool main_recorded = false;
  int count_kernel = GAT_COUNT_KERNEL_NONE;
  // k_units_overlap (CountArgs::cu_rec set): the units and their workspaces
  const gat::UnitDev* units = nullptr;
  const uint2* ws = nullptr;
  const uint32_t* ws_tree = nullptr;
  int max_units = 1;          // ... the most units a contig has
};
// n launch positions spread over grid y and z (each <= 65535) behind the x the kernel asks for
static inline dim3 grid_yz(unsigned x, unsigned n) {
  const unsigned gy = std::min(n, 32768u);
  return dim3(x, gy, (n + gy - 1) / std::max(gy, 1u));
}

static int launch_count(gat_ctx* ctx, const Knobs& kn, const AnnoDev& annos, const Counters& C, gat::CountArgs A, DevBuf<uint32_t>& part,
                        int swap_capx, int list_cap, CountLaunch& L) {
  L.main_recorded = false;
  L.count_kernel = GAT_COUNT_KERNEL_NONE;
  gat_count_report& R = ctx->count_report;      // (what is launched below, for gat_count_last_launch: no launch depends on it)
  R = gat_count_report();
  for (int i = 0; i < GAT_NUM_COUNTERS; ++i) A.counter_slot[i] = C.slot[i];
  A.a_start = annos.start.p; A.a_end = annos.end.p; A.a_cumx = annos.cumx.p; A.a_off = annos.off.p;
  A.a_grid = annos.grid.p; A.g_off = annos.goff.p; A.c_shift = annos.shift.p; A.c_cells = annos.cells.p;
  if (A.n_samples <= 0 || A.n_tracks <= 0) return GAT_OK;
  if (!annos.per_track && (C.any_anno || (C.any_seg && count_route(ctx, kn, annos.has_merged, C, A.n_contigs, A.n_tracks, swap_capx, true) != GAT_COUNT_KERNEL_MERGED)))
    return set_err(ctx, GAT_ERR_ARG, "the annotation tables were made for the nucleotide counters only (GAT_ANNOTATIONS_NUCLEOTIDE_ONLY): "
                                     "no per-track tables for the counters asked for");
  if (C.any_seg) {
    const int E_max = (int)kn.count_lds_entries;
    int SC = (int)kn.count_samples_per_block;
    if (!kn.count_samples_per_block_set) {   // enough blocks to fill 256 CUs several times over, large enough to amortise the staging
      const int64_t tiles0 = (A.n_tracks + 0) , work = (int64_t)A.n_samples * tiles0 * std::max(1, A.n_contigs) / 8192;
      SC = 8;
      while (SC < 128 && SC * 2 <= work) SC *= 2;
    }
    SC = std::max(1, std::min(SC, 256));
    const int TT_max = (int)kn.count_tracks_per_block;
    int TT;
    // (+4: a staged list has an entry in front of its first interval and three sentinels behind the last: segs_vs_pairs)
    bool staged = count_lists_staged(kn, annos.max_m) && (int)kn.count_staged != 0;
    if (staged) TT = (int)std::min<int64_t>(std::min<int64_t>(A.n_tracks, TT_max), E_max / (annos.max_m + 4));
    else TT = (int)std::min<int64_t>(A.n_tracks, TT_max);
    TT = std::max(1, TT);
    A.tracks_per_block = TT;
    A.samples_per_block = SC;
    A.lds_entries = staged ? (int)std::min<int64_t>((int64_t)E_max, (annos.max_m + 4) * TT) : 0;
    A.lds_grid = staged ? (int)((annos.max_cells + 1) * TT) : 0;
    const size_t lds = (size_t)((TT + 1 + 3) & ~3) * 4 + (size_t)3 * A.lds_entries * 4 + (size_t)A.lds_grid * 4;
    const size_t need = (size_t)A.n_contigs * 3 * (size_t)A.n_tracks * (size_t)A.n_samples;
    if (part.n < need) HIPCHK(ctx, part.alloc(need));
    A.part = part.p;
    // (track tile, contig) pairs over grid y and z, contigs alone likewise for the kernels gridded by contig
    const int64_t n_pairs = (int64_t)((A.n_tracks + TT - 1) / TT) * std::max(1, A.n_contigs);
    const unsigned gpy = (unsigned)std::min<int64_t>(n_pairs, 32768), gpz = (unsigned)((n_pairs + gpy - 1) / gpy);
    if (gpz > 65535) return set_err(ctx, GAT_ERR_CAPACITY, "more than 2^31 (track tile, contig) pairs");
    dim3 grid((unsigned)((A.n_samples + SC - 1) / SC), gpy, gpz);
    const size_t lds_merged = (size_t)A.n_tracks * 4 * (gat::kMergedThreads / gat::kWave);
    const int route = count_route(ctx, kn, annos.has_merged, C, A.n_contigs, A.n_tracks, swap_capx, !annos.per_track);
    if (route == GAT_COUNT_KERNEL_MERGED) {
      // several tracks: one look-up per sample segment in the merged index of all tracks
      A.mz = annos.mz.p; A.mz_off = annos.mz_off.p; A.mfirst = annos.mfirst.p; A.mf_off = annos.mf_off.p;
      A.m_shift = annos.m_shift.p; A.m_cells = annos.m_cells.p;
      A.m_slot_off = annos.m_slot_off.p; A.m_slot_contigs = annos.m_slot_contigs.p;
      // samples per workgroup: one per wave.  (Larger groups were meant to keep the contig's index hot; measured on config 3,
      // main kernel per 10 000 samples: 4 -> 1.60 ms, 8 -> 1.69, 16 -> 1.73, 32 -> 1.83, 64 -> 2.1: the finer deal wins.)
      int SG = (int)kn.merged_samples_per_block;
      SG = std::max(1, std::min(SG, std::max(1, A.n_samples)));
      A.samples_per_block = SG;
      const int64_t n_sgroups = (A.n_samples + SG - 1) / SG;
      const int64_t nblocks = (int64_t)gat::kMergedSlots * annos.max_slot_contigs * n_sgroups;
      if (nblocks >= ((int64_t)1 << 31)) return set_err(ctx, GAT_ERR_CAPACITY, "more than 2^31 (contig, sample group) pairs");
      const size_t need = (size_t)A.n_contigs * (size_t)A.n_tracks * (size_t)A.n_samples;
      if (part.n < need) HIPCHK(ctx, part.alloc(need));
      A.part = part.p;
      const bool patch = A.seg_merged != nullptr;
      const int blk = annos.merged_block;
      A.mcell = annos.mcell.p;
      const void* km = patch ? (blk == 8 ? (const void*)gat::k_count_merged<true, 8> : blk == 1 ? (const void*)gat::k_count_merged<true, 1>
                                                                                                 : (const void*)gat::k_count_merged<true, 2>)
                             : (blk == 8 ? (const void*)gat::k_count_merged<false, 8> : blk == 1 ? (const void*)gat::k_count_merged<false, 1>
                                                                                                  : (const void*)gat::k_count_merged<false, 2>);
      HIPCHK(ctx, hipFuncSetAttribute(km, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_merged));
      HIPCHK(ctx, hipEventRecord(L.ev_main[0], L.stream));
      const dim3 gm((unsigned)nblocks), bm(gat::kMergedThreads);
      if (patch && blk == 8) hipLaunchKernelGGL((gat::k_count_merged<true, 8>), gm, bm, lds_merged, L.stream, A);
      else if (patch && blk == 1) hipLaunchKernelGGL((gat::k_count_merged<true, 1>), gm, bm, lds_merged, L.stream, A);
      else if (patch) hipLaunchKernelGGL((gat::k_count_merged<true, 2>), gm, bm, lds_merged, L.stream, A);
      else if (blk == 8) hipLaunchKernelGGL((gat::k_count_merged<false, 8>), gm, bm, lds_merged, L.stream, A);
      else if (blk == 1) hipLaunchKernelGGL((gat::k_count_merged<false, 1>), gm, bm, lds_merged, L.stream, A);
      else hipLaunchKernelGGL((gat::k_count_merged<false, 2>), gm, bm, lds_merged, L.stream, A);
      HIPCHK(ctx, hipGetLastError());
      if (A.cu_rec != nullptr) {
        // the contig lists were only concatenated (k_contig<., true>): what fromIsochores would have united -- the overlaps
        // between different units' segments -- off the partial sums again
        gat::UnitsOverlapArgs B;
        B.C = A; B.units = L.units; B.ws = L.ws; B.ws_tree = L.ws_tree;
        const int64_t items = (int64_t)A.cand_cap * std::max(1, L.max_units);
        hipLaunchKernelGGL(gat::k_units_overlap, dim3((unsigned)((items + 255) / 256), gat::kCandSlots), dim3(256), 0, L.stream, B,
                           std::max(1, L.max_units));
        HIPCHK(ctx, hipGetLastError());
      }
      HIPCHK(ctx, hipEventRecord(L.ev_main[1], L.stream));
      L.main_recorded = true;
      L.count_kernel = GAT_COUNT_KERNEL_MERGED;
      R.kernel = GAT_COUNT_KERNEL_MERGED; R.patch = patch ? 1 : 0; R.samples_per_block = SG;
      R.merged_form = blk == 8 ? 8 : blk == 1 ? 1 : 2;
      const int64_t tiles = (int64_t)((A.n_tracks + 15) / 16) * ((A.n_samples + 15) / 16);
      hipLaunchKernelGGL(gat::k_count_merged_finish, dim3((unsigned)tiles), dim3(256), 0, L.stream, A);
      HIPCHK(ctx, hipGetLastError());
      goto seg_done;
    }
    if (route == GAT_COUNT_KERNEL_SWAP) {
      // long sample lists against short annotation lists: index the sample list, stream the tracks
      gat::CountArgs B = A;
      int lcells = 4;
      while ((1 << lcells) < swap_capx && lcells < 13) ++lcells;
      B.lds_entries = swap_capx;
      B.lds_grid = lcells;
      const size_t lds_swap = (size_t)3 * swap_capx * 4 + ((size_t)(1 << lcells) + 1) * 4;
      HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_count_swap, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_swap));
      HIPCHK(ctx, hipEventRecord(L.ev_main[0], L.stream));
      hipLaunchKernelGGL(gat::k_count_swap, grid_yz((unsigned)A.n_samples, (unsigned)std::max(1, A.n_contigs)), dim3(gat::kSwapThreads), lds_swap, L.stream, B);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipEventRecord(L.ev_main[1], L.stream));
      L.main_recorded = true;
      L.count_kernel = GAT_COUNT_KERNEL_SWAP;
      R.kernel = GAT_COUNT_KERNEL_SWAP;
    } else
    if (A.n_contigs > 0) {
    const bool hits = C.slot[GAT_COUNTER_SEGMENT_OVERLAP] >= 0 || C.slot[GAT_COUNTER_SEGMENT_MIDOVERLAP] >= 0;
    HIPCHK(ctx, hipEventRecord(L.ev_main[0], L.stream));
    const int kv = (staged ? 4 : 0) + (hits ? 2 : 0) + (A.seg_merged != nullptr ? 1 : 0);
    typedef void (*count_fn)(gat::CountArgs);
    static const count_fn kCountSegFns[8] = {
        gat::k_count_seg<false, false, false>, gat::k_count_seg<false, false, true>, gat::k_count_seg<false, true, false>,
        gat::k_count_seg<false, true, true>, gat::k_count_seg<true, false, false>, gat::k_count_seg<true, false, true>,
        gat::k_count_seg<true, true, false>, gat::k_count_seg<true, true, true>};
    if (staged) HIPCHK(ctx, hipFuncSetAttribute((const void*)kCountSegFns[kv], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kCountSegFns[kv], grid, dim3(256), lds, L.stream, A);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(L.ev_main[1], L.stream));
    L.main_recorded = true;
    L.count_kernel = GAT_COUNT_KERNEL_SEG;
    R.kernel = GAT_COUNT_KERNEL_SEG; R.staged = staged ? 1 : 0; R.hits = hits ? 1 : 0; R.patch = A.seg_merged != nullptr ? 1 : 0;
    R.tracks_per_block = TT; R.samples_per_block = SC;
    }
    {
      const int64_t nfin = (int64_t)A.n_tracks * A.n_samples;
      hipLaunchKernelGGL(gat::k_count_finish, dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, L.stream, A);
      HIPCHK(ctx, hipGetLastError());
    }
  seg_done:;
  }
  if (C.any_anno) {
    // the sample lists indexed in LDS when they fit (list_cap = longest list possible), else every interval bisects
    // the list in global memory
    int lcells = 4;
    while ((1 << lcells) < list_cap + 1 && lcells < 13) ++lcells;
    const size_t lds_a = (size_t)2 * (list_cap + 1) * 4 + ((size_t)(1 << lcells) + 1) * 4;
    if (list_cap > 0 && A.n_contigs > 0 && (int64_t)lds_a + 1024 <= ctx->max_lds && !kn.count_no_swap) {
      gat::CountArgs B = A;
      B.lds_entries = list_cap + 1;
      B.lds_grid = lcells;
      const size_t need = (size_t)A.n_contigs * 2 * (size_t)A.n_tracks * (size_t)A.n_samples;
      if (part.n < need) HIPCHK(ctx, part.alloc(need));
      B.part = part.p;
      HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_count_anno_idx, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
      hipLaunchKernelGGL(gat::k_count_anno_idx, grid_yz((unsigned)A.n_samples, (unsigned)A.n_contigs), dim3(gat::kAnnoThreads), lds_a, L.stream, B);
      HIPCHK(ctx, hipGetLastError());
      const int64_t nfin = (int64_t)A.n_tracks * A.n_samples;
      hipLaunchKernelGGL(gat::k_count_anno_finish, dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, L.stream, B);
      HIPCHK(ctx, hipGetLastError());
      R.anno_kernel = GAT_COUNT_ANNO_IDX;
    } else {
      const int64_t waves = (int64_t)A.n_samples * A.n_tracks;
      hipLaunchKernelGGL(gat::k_count_anno, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, L.stream, A);
      HIPCHK(ctx, hipGetLastError());
      R.anno_kernel = GAT_COUNT_ANNO_PLAIN;
    }
  }
  return GAT_OK;
}

// sampler (+ fromIsochores) for one batch; retries with a larger slab on overflow
// Returns GAT_OK, an error, or kRelayout: a unit's region overflowed, the slab was laid out again with doubled
// capacities (scratch released: the batch that fits the budget may now be smaller) and nothing of this batch is valid;
// the caller sizes the batch again and repeats it (results do not depend on the batching: streams are per unit).
constexpr int kRelayout = 1;

// what a caller of run_sampler_batch asks for beyond the defaults
struct BatchOpts {
  bool need_unit_lists = false;          // somebody reads the units' final lists (gat_sample_units): written whoever counts
  bool defer = false;                    // only enqueue (the caller adds the count kernels behind, synchronises once and calls finish_sampler_batch)
  bool records_ok = false;               // the consumer is k_count_seg alone, which reads (merged list, k_tail's record): no k_finalize
  uint32_t* serial_state = nullptr;      // the run's ONE MT19937 state on the device (k_serial: the reference's own stream) instead of the per-unit streams
  bool loose_ok = false;                 // the consumer skips empty segments (k_count_merged): long lists may keep what a trim emptied
  unsigned long long* h_stat = nullptr;  // the pinned words the batch's statistics are copied to (nullptr: the context's)
  // an isochore problem whose counters (the nucleotide counters, through the merged index) take the units' lists as the sampler
  // leaves them: no k_contig (k_count_merged<2, .> + k_units_overlap; P->units_direct says whether the batch took it)
  bool units_direct = false;
};

// One batch's decisions -- which stages run, and the sizes they share -- made once (plan_batch) from the problem, the context's
// knobs and the caller's options; read-only for the stages.  What a stage leaves for the kernels behind it, it adds to the
// batch's SamplerArgs.
struct BatchPlan {
  const Knobs& kn;         // the call's snapshot of the knobs
  BatchOpts o;
  int64_t nb; bool timed;
  unsigned n_act;          // active units: the launch positions
  uint32_t max_work;       // the largest hist_total of the active units
  int smode;               // 0: the reference's own stream (k_serial), no front end
  bool huge;               // a SamplerAnnotator list beyond LDS is worked on in the slab (HUGE variant); SamplerSegments never holds a list
  bool tree;               // workspaces beyond the register loop: search trees
  bool split;              // the split path (k_consolidate / k_merge_big + k_tail + k_finalize in front of k_sampler); lists beyond LDS: old path
  bool long_lists;         // k_sampler<BIG>: the code for lists beyond the bucket sorts
  unsigned n_long;         // the long units, which come first in the launch order
  int nbk;                 // histogram buckets for the longest list (a power of two, 1 024 .. 8 192)
  size_t lds_merge;        // the most k_merge_big takes: its LDS holds one list and the counting sort's histogram
  bool merge_big;          // the first consolidation of the long lists by whole workgroups, launched over the n_long units
  bool tail_big;           // ... the placement rounds behind it, one stream per lane (k_tail_big)
  bool resume_big;         // ... and the rest of the unit with the list where it is (k_resume_big)
  bool long_queue;         // ... with k_sampler working off a queue (k_queue_rest)
  int big_buckets;         // no workgroup pass: the wave's own counting sort, its scratch behind k_sampler's segment buffer (0: none)
  size_t lds;              // k_sampler's LDS for the longest list
};

static BatchPlan plan_batch(const gat_ctx* ctx, const Knobs& kn, const gat_problem* P, int64_t nb, bool timed, const BatchOpts& o) {
  BatchPlan B = {kn};
  B.o = o; B.nb = nb; B.timed = timed;
  B.n_act = (unsigned)P->h_order.size();
  for (int32_t u : P->h_order) B.max_work = std::max(B.max_work, P->h_units[(size_t)u].hist_total);
  B.smode = o.serial_state != nullptr ? 0 : P->sampler_mode;
  B.lds = (size_t)(gat::kMtLdsWords + 2 * (size_t)P->max_unit_cap) * 4;
  B.huge = P->sampler != GAT_SAMPLER_SEGMENTS && ((int64_t)B.lds > ctx->max_lds || kn.test_huge);
  if (B.huge || P->sampler == GAT_SAMPLER_SEGMENTS) B.lds = (size_t)gat::kMtLdsWords * 4;
  B.tree = P->max_nws > gat::kWsTreeMin;
  B.split = P->split_path && B.smode && !B.huge;
  B.long_lists = !B.huge && B.max_work + B.max_work / 8 > 1024;
  if (!B.long_lists) return B;
  B.nbk = 1024;
  while (B.nbk < P->max_unit_cap && B.nbk < 8192) B.nbk <<= 1;
  B.lds_merge = (size_t)2 * P->max_unit_cap * 4 + (size_t)(B.nbk + 1) * 4;
  for (int32_t u : P->h_order) { const uint32_t w = P->h_units[(size_t)u].hist_total; if (w + w / 8 > 1024) ++B.n_long; else break; }
  B.merge_big = B.smode && P->sampler != GAT_SAMPLER_SEGMENTS && (int64_t)B.lds_merge + 1024 <= ctx->max_lds && B.n_long > 0 &&
                !kn.no_merge_big;
  if (B.merge_big) {
    B.tail_big = !B.split && P->d_patch.p != nullptr && P->max_nws <= gat::kTailMaxWs && !kn.no_tail_big;
    B.resume_big = B.tail_big && !kn.no_resume_big;
    B.long_queue = B.resume_big && !kn.no_long_queue;
  } else {
    // no workgroup pass: the wave's own counting sort, scratch behind the segment buffer if it fits
    int nbk = B.nbk;
    while (nbk >= 1024 && (int64_t)(B.lds + (size_t)(nbk + 1) * 4) > ctx->max_lds) nbk >>= 1;
    if (nbk >= 1024) { B.big_buckets = nbk; B.lds += (size_t)(nbk + 1) * 4; }
  }
  return B;
}

// The plan as gat_sampler_last_launch reports it: the stages below add what they launch per size class.  No launch reads it.
static void record_plan(gat_ctx* ctx, const gat_problem* P, const BatchPlan& B) {
  gat_sampler_report& R = ctx->sampler_report;
  R = gat_sampler_report();
  R.sampler_variant = -1;
  if (sampler_runs_wave_per_unit(P->sampler)) return;      // (one kernel, no stages: nothing of the plan applies)
  R.huge = B.huge; R.split = B.split; R.long_lists = B.long_lists; R.tree = B.tree;
  R.merge_big = B.merge_big; R.tail_big = B.tail_big; R.resume_big = B.resume_big; R.long_queue = B.long_queue;
  R.big_buckets = B.big_buckets; R.n_long = (int32_t)B.n_long;
  R.n_classes = (int32_t)P->h_class_start.size() - 1;
  for (int c = 0; c < R.n_classes && c < GAT_SAMPLER_REPORT_CLASSES; ++c) {
    R.cls[c].first = P->h_class_start[(size_t)c];
    R.cls[c].merge_form = -1;
  }
}

// The wave-per-unit samplers that write the units' final (normalized) lists -- no front end, no split path, no records: what
// their argument structs share, the grid and the launch.  H comes with the sampler's own tables and lds_cap.
template <typename Args>
static int enqueue_list_sampler(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin,
                                void (*kernel)(Args), Args& H, size_t lds) {
  H.units_o = P->d_units_o.p; H.n_units = P->n_units; H.n_active = (int32_t)B.n_act;
  H.rec_stride = (int32_t)P->batch;
  H.seed = seed; H.sample_begin = begin;
  H.slab = P->d_slab.p; H.slab_stride = P->slab_stride;
  H.unit_n = P->d_unit_n.p; H.flags = P->flags_dev(); H.ws_stat = P->d_ws_stat.p;
  HIPCHK(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid_yz((unsigned)B.nb, B.n_act), dim3(64), lds, call_stream(ctx, P), H);
  HIPCHK(ctx, hipGetLastError());
  return GAT_OK;
}

// SamplerShift: k_shift
static int enqueue_shift(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin) {
  gat::ShiftArgs H;
  memset(&H, 0, sizeof(H));
  // (LDS for the list a unit is expected to leave -- about one piece per segment, a quarter + 64 on top -- not for its slab
  //  region: LDS is what bounds the waves a CU holds, and the kernel is a chain of dependent loads; a longer list is sorted
  //  and merged in the slab)
  H.lds_cap = std::min<int32_t>(std::min(P->max_unit_cap, 2048), (int32_t)(B.max_work + B.max_work / 4 + 64));
  H.ws = P->d_ws.p; H.ws_cdf = P->d_ws_cdf.p; H.shift = P->d_shift.p; H.shift_off = P->d_shift_off.p;
  H.stat = P->d_stat.p;
  return enqueue_list_sampler(ctx, P, B, seed, begin, gat::k_shift, H, (size_t)(gat::kMtLdsWords + 2 * (size_t)H.lds_cap) * 4);
}

// SamplerGlobalPermutation: k_permute
static int enqueue_permute(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin) {
  gat::PermuteArgs H;
  memset(&H, 0, sizeof(H));
  // (LDS for the lengths and the points of the longest unit, up to 2 048 working segments -- 24 KB with the generator's
  //  state; a longer unit keeps them in its slab region)
  H.lds_cap = (int32_t)std::min<uint32_t>(B.max_work, 2048u);
  H.perm_unit = P->d_perm_unit.p; H.perm_len = P->d_perm_len.p; H.perm_w = P->d_perm_w.p; H.perm_cum = P->d_perm_cum.p;
  return enqueue_list_sampler(ctx, P, B, seed, begin, gat::k_permute, H,
                              (size_t)(gat::kMtLdsWords + ((H.lds_cap + 1) & ~1) + 2 * (size_t)H.lds_cap) * 4);
}

// SamplerLocalPermutation: k_permute_local
static int enqueue_permute_local(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin) {
  gat::LocalPermuteArgs H;
  memset(&H, 0, sizeof(H));
  // (LDS for the lengths and points of the largest piece, up to 2 048 working segments, and -- the same words -- for the final
  //  list of up to 2 048 pieces: 3 KB for a fragmented workspace of one or two segments per piece, where the kernel is the
  //  chain of the pieces' draws and the waves a CU holds are what hides it; 27 KB at most.  A larger piece keeps its arrays
  //  in the slab, a longer list is sorted and merged there)
  H.lds_cap = std::max(64, std::min(P->lperm_max_n, 2048));
  const int32_t words = std::max<int32_t>(((H.lds_cap + 1) & ~1) + 2 * H.lds_cap, 2 * (int32_t)std::min<int64_t>(P->lperm_max_out, 2048));
  H.list_cap = words / 2;
  H.lp_unit = P->d_lperm_unit.p; H.lp_piece = P->d_lperm_piece.p; H.lp_len = P->d_lperm_len.p;
  // (GAT_LPERM_SIMPLE: one piece per wave step throughout, the A/B of the batched small-piece path;
  //  GAT_EXP_LPERM_NO_NORMALIZE: a timing experiment with wrong results -- no final sort and merge, empty lists)
  H.simple = B.kn.lperm_simple ? 1 : 0;
  H.no_normalize = B.kn.exp_lperm_no_normalize ? 1 : 0;
  return enqueue_list_sampler(ctx, P, B, seed, begin, gat::k_permute_local, H,
                              (size_t)(gat::kMtLdsWords + 2 * gat::kLpBatchDraws + words) * 4);
}

// SamplerCircular: k_circular
static int enqueue_circular(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin) {
  gat::CircularArgs H;
  memset(&H, 0, sizeof(H));
  H.ws = P->d_ws.p; H.ws_cdf = P->d_ws_cdf.p; H.circ_unit = P->d_circ_unit.p; H.circ_iv = P->d_circ_iv.p;
  // (LDS for the generator's state alone: the intervals are read where they lie and the pieces go straight to the slab)
  return enqueue_list_sampler(ctx, P, B, seed, begin, gat::k_circular, H, (size_t)gat::kMtLdsWords * 4);
}

// SamplerUniverse: k_universe
static int enqueue_universe(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin) {
  gat::UniverseArgs H;
  memset(&H, 0, sizeof(H));
  H.ws = P->d_ws.p; H.univ_unit = P->d_univ_unit.p;
  // (LDS for the generator's state and the mark table of the largest active unit, one bit per piece in whole wave steps:
  //  the kernel is the chain of the marks' test-and-set steps, hidden by the waves a CU holds, and LDS is what bounds them.
  //  Problem creation refused what the context's LDS does not hold)
  H.table_words = (int32_t)P->univ_table_words;
  const size_t lds = (size_t)gat::kUniverseFixedLdsBytes + (size_t)H.table_words * 4;
  if ((int64_t)lds > ctx->max_lds) return set_err(ctx, GAT_ERR_CAPACITY, "SamplerUniverse: a mark table of %d words", (int)H.table_words);
  return enqueue_list_sampler(ctx, P, B, seed, begin, gat::k_universe, H, lds);
}

// SamplerBruteForce: k_brute_force
static int enqueue_brute_force(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin) {
  gat::BruteForceArgs H;
  memset(&H, 0, sizeof(H));
  // (LDS for the first kBruteLdsCap accepted segments -- the kernel is a chain of dependent draws, hidden by the waves a CU
  //  holds, and LDS is what bounds them; a longer list goes on in the unit's slab region)
  H.lds_cap = std::max<int32_t>(64, std::min<int32_t>(P->max_unit_cap, gat::kBruteLdsCap));
  H.ntries_inner = P->brute_ntries_inner; H.ntries_outer = P->brute_ntries_outer;
  H.ws = P->d_ws.p; H.ws_cdf = P->d_ws_cdf.p; H.rank_len = P->d_rank_len.p;
  H.stat = P->d_stat.p;
  HIPCHK(ctx, hipMemsetAsync(P->d_stat.p + gat::kStatBruteFirst, 0, 8, call_stream(ctx, P)));
  return enqueue_list_sampler(ctx, P, B, seed, begin, gat::k_brute_force, H, (size_t)(gat::kMtLdsWords + 2 * (size_t)H.lds_cap) * 4);
}

// the arguments every kernel of SamplerAnnotator / SamplerSegments starts from
static int base_sampler_args(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin, gat::SamplerArgs& A) {
  memset(&A, 0, sizeof(A));
  A.units = P->d_units.p; A.units_o = P->d_units_o.p; A.order = P->d_order.p; A.n_units = P->n_units; A.batch = (int32_t)B.nb;
  A.rec_stride = (int32_t)P->batch;                  // (the scratch's size in samples: the records' row length in every batch)
  A.ws = P->d_ws.p; A.ws_cdf = P->d_ws_cdf.p; A.rank_len = P->d_rank_len.p; A.ws_tree = P->d_ws_tree.p;
  A.ws_rec = P->d_ws_rec.p;
  A.seed = seed; A.sample_begin = begin; A.sampler_kind = P->sampler;
  A.place_plain_step = B.kn.place_no_cm ? 1 : 0;
  A.slab = P->d_slab.p; A.slab_stride = P->slab_stride;
  A.unit_n = P->d_unit_n.p; A.flags = P->flags_dev(); A.stat = P->d_stat.p; A.ws_stat = P->d_ws_stat.p;
#if defined(GAT_DIAG) || defined(GAT_DIAG_CONS)
  {
    const size_t nd = (size_t)B.nb * std::max(1, P->n_units) * 8;
    if (P->d_diag.n < nd) HIPCHK(ctx, P->d_diag.alloc(nd));
    HIPCHK(ctx, hipMemsetAsync(P->d_diag.p, 0, nd * 8, call_stream(ctx, P)));
    A.diag = P->d_diag.p;
  }
#endif
#ifdef GAT_DIAG
  {
    const size_t np = std::max<size_t>(1, P->h_order.size()) * 8;
    if (P->d_diag_place.n < np) HIPCHK(ctx, P->d_diag_place.alloc(np));
    HIPCHK(ctx, hipMemsetAsync(P->d_diag_place.p, 0, np * 8, call_stream(ctx, P)));
    A.diag_place = P->d_diag_place.p;
    const size_t nt = std::max<size_t>(1, P->h_order.size()) * (size_t)((B.nb + 63) / 64) * 2;
    if (P->d_diag_tiles.n < nt) HIPCHK(ctx, P->d_diag_tiles.alloc(nt));
    HIPCHK(ctx, hipMemsetAsync(P->d_diag_tiles.p, 0, nt * 8, call_stream(ctx, P)));
    A.diag_tiles = P->d_diag_tiles.p;
  }
#endif
  A.n_active = (int32_t)B.n_act;
  if (B.smode) {
    A.rng_off = P->d_rng_off.p; A.rng_rows = P->d_rng_rows.p; A.rng_out = P->d_rng_out.p;
    A.rng_ckpt = P->d_rng_ckpt.p;
    A.st = P->d_st.p;
  }
  return GAT_OK;
}

// the one k_place* kernel of a batch: nsb tiles of 64 samples per unit
static int launch_place(gat_ctx* ctx, const gat_problem* P, const BatchPlan& B, const gat::SamplerArgs& A, unsigned nsb) {
  const dim3 gp = grid_yz(nsb, B.n_act);
  // (small calls of a problem of simple units -- about a wave per SIMD or less, e.g. the metric's 10 000 samples cut over
  //  eight GPUs -- take the wide kernel as well: its loop stores unconditionally and four tiles share a rank table; config 2,
  //  k_place at 1 250 / 2 500 / 5 000 samples: 0.46 / 0.47 / 0.56 ms against the lean kernel's 0.52 / 0.53 / 0.57, at 10 000
  //  1.05 against 0.92)
  const bool small_call = (int64_t)nsb * (int64_t)B.n_act <= 1536 && !B.kn.place_no_wide;
  const int mode = P->all_simple ? ((B.kn.place_wide || small_call) ? 3 : 1)
                                 : (P->all_one_ws && !B.kn.place_no_wide ? 3 : (P->max_nws > gat::kPlaceWsLds ? 2 : 0));
  // (k_place_wide: kPlaceWide tiles per workgroup, the largest unit's rank table beside their rings)
  const dim3 gw = grid_yz((nsb + gat::kPlaceWide - 1) / gat::kPlaceWide, B.n_act);
  const size_t lds_wide = (size_t)P->max_hist * 4;
  // calls of a few hundred tiles of a problem of simple units: one stream walked by the 64 lanes of a wave (k_place_scan:
  // a stream's states as a prefix scan over its rows) instead of one lane walking it row by row -- the chain of the longest
  // unit's tile, 0.37 ms on config 2 whatever the sample count, is what such a call waited for
  const int64_t scan_tiles = B.kn.place_scan_tiles;                 // (config 2: faster up to ~2 300 samples x 24 units per call)
  const bool scan = P->sampler == GAT_SAMPLER_ANNOTATOR && P->all_simple && P->all_cm_ok && A.place_plain_step == 0 &&
                    (int64_t)nsb * (int64_t)B.n_act <= scan_tiles;
  if (scan) {
    const int64_t n_tiles = (int64_t)nsb * B.n_act;
    const unsigned nblocks = (unsigned)(((n_tiles + 7) / 8) * 8 * 4);
    hipLaunchKernelGGL(gat::k_place_scan, dim3(nblocks), dim3(gat::kScanWaves * 64), 0, call_stream(ctx, P), A, (int)nsb,
                       B.kn.place_scan_seq ? 1 : 0);
  } else if (P->sampler == GAT_SAMPLER_SEGMENTS) {
    if (mode == 3) {
      HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_place_wide<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wide));
      hipLaunchKernelGGL((gat::k_place_wide<1>), gw, dim3(gat::kPlaceWide * 64), lds_wide, call_stream(ctx, P), A);
    } else if (mode == 1) hipLaunchKernelGGL((gat::k_place<1, 1>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0) hipLaunchKernelGGL((gat::k_place<1, 0>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else hipLaunchKernelGGL((gat::k_place<1, 2>), gp, dim3(64), 0, call_stream(ctx, P), A);
  } else {
    // (k_place_pipe: the rows of the single-workspace-segment units prefetched by hand, see GAT_PLACE_LOOP_PIPE)
    const bool pipe = P->pipe_pays && !B.kn.place_no_pipe;
    const bool rank_fits = P->max_hist < (uint32_t)gat::kPlaceRankLds;
    // fragmented workspaces: the cdf grids of the long workspaces in LDS, eight tiles of a unit per workgroup (k_place_grid);
    // static LDS: the workspace and rank tables (4 KB each) and an 8 KB ring per tile
    const size_t lds_grid = (size_t)P->grid_lds_words * 4 + 16;
    const bool grid_k = mode == 2 && P->grid_place && (int64_t)lds_grid + 8192 + 1024 + (int64_t)gat::kPlaceGridTiles * 8192 <= ctx->max_lds;
    if (grid_k) {
      HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_place_grid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_grid));
      hipLaunchKernelGGL(gat::k_place_grid, grid_yz((nsb + gat::kPlaceGridTiles - 1) / gat::kPlaceGridTiles, B.n_act),
                         dim3(gat::kPlaceGridTiles * 64), lds_grid, call_stream(ctx, P), A);
    } else if (mode == 3) {
      HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_place_wide<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wide));
      hipLaunchKernelGGL((gat::k_place_wide<0>), gw, dim3(gat::kPlaceWide * 64), lds_wide, call_stream(ctx, P), A);
    } else if (mode == 1 && pipe) hipLaunchKernelGGL((gat::k_place_pipe<0, 1>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 1) hipLaunchKernelGGL((gat::k_place<0, 1>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0 && P->small_tables && pipe) hipLaunchKernelGGL((gat::k_place_pipe<0, 0, 1>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0 && P->small_tables) hipLaunchKernelGGL((gat::k_place<0, 0, 1>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0 && P->max_nws <= 64 && rank_fits && pipe) hipLaunchKernelGGL((gat::k_place_pipe<0, 0, 2>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0 && P->max_nws <= 64) hipLaunchKernelGGL((gat::k_place<0, 0, 2>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0 && rank_fits && pipe) hipLaunchKernelGGL((gat::k_place_pipe<0, 0>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else if (mode == 0) hipLaunchKernelGGL((gat::k_place<0, 0>), gp, dim3(64), 0, call_stream(ctx, P), A);
    else hipLaunchKernelGGL((gat::k_place<0, 2>), gp, dim3(64), 0, call_stream(ctx, P), A);
  }
  HIPCHK(ctx, hipGetLastError());
  return GAT_OK;
}

// The lane-parallel front end: the streams (k_seed, k_rng) and every placement up to the first consolidation (k_place*).  The
// scratch was sized for P->batch samples, tiles are laid out for that.
static int enqueue_front_end(gat_ctx* ctx, const gat_problem* P, const BatchPlan& B, const gat::SamplerArgs& A) {
  const unsigned nsb = (unsigned)((B.nb + 63) / 64);
  // the streams' seeding chains at full occupancy, 16 checkpoints each; k_rng's waves regenerate the rest
  const int64_t n_tiles = (int64_t)nsb * B.n_act, per_block = gat::kSeedThreads / gat::kWave;
  hipLaunchKernelGGL(gat::k_seed, dim3((unsigned)((n_tiles + per_block - 1) / per_block)), dim3(gat::kSeedThreads), 0, call_stream(ctx, P),
                     A, (int)nsb);
  HIPCHK(ctx, hipGetLastError());
  const size_t lds_rng = (size_t)gat::kMtN * 64 * 4;
  HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_rng, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rng));
  hipLaunchKernelGGL(gat::k_rng, grid_yz(nsb, B.n_act), dim3(gat::kRngThreads), lds_rng, call_stream(ctx, P), A);
  HIPCHK(ctx, hipGetLastError());
  if (B.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k[0], call_stream(ctx, P)));
  const int rc = launch_place(ctx, P, B, A, nsb);
  if (rc) return rc;
  if (B.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k[1], call_stream(ctx, P)));
  return GAT_OK;
}

// The long-list chain (B.merge_big): k_merge_big per size class, then -- without the split path -- k_tail_big, k_resume_big and
// k_queue_rest.  Adds to A what k_sampler (and the split path) read of it: st2 / n_long, k_tail_big's records, the queue.
static int enqueue_long_lists(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, gat::SamplerArgs& A) {
  const unsigned n_long = B.n_long;
  gat::SamplerArgs M = A;
  M.st2 = P->d_st2.p; M.n_long = (int32_t)n_long;
  M.big_buckets = B.nbk;
  M.cum = B.split ? P->d_cum.p : nullptr;
  // (the form by the class's longest list: 8, 16 or 24 elements of it in every thread's registers; 0 = round 3's form,
  //  the list read twice and sorted bucket by bucket)
  typedef void (*merge_fn)(gat::SamplerArgs);
  static const merge_fn kMergeFns[2][4] = {
      {gat::k_merge_big<false, 0>, gat::k_merge_big<false, 8>, gat::k_merge_big<false, 16>, gat::k_merge_big<false, gat::kMergeRegs>},
      {gat::k_merge_big<true, 0>, gat::k_merge_big<true, 8>, gat::k_merge_big<true, 16>, gat::k_merge_big<true, gat::kMergeRegs>}};
  const merge_fn* fns = kMergeFns[B.tree ? 1 : 0];
  const bool merge_old = B.kn.merge_old;
  for (int f = 0; f < 4; ++f)
    HIPCHK(ctx, hipFuncSetAttribute((const void*)fns[f], hipFuncAttributeMaxDynamicSharedMemorySize, (int)B.lds_merge));
  for (size_t c = 0; c + 1 < P->h_class_start.size() && (unsigned)P->h_class_start[c] < n_long; ++c) {
    // one launch per size class: LDS for the class's longest list and its histogram
    const int a0 = P->h_class_start[c], a1 = std::min<int>(P->h_class_start[c + 1], (int)n_long);
    // LDS for what the class's longest unit is EXPECTED to have placed at its first consolidation, not for its slab
    // region (a quarter + 96 above the unit's segments): the count of placements is the unit's segments +- a
    // renewal count's spread, cv(length) x sqrt(n) -- 90 for 8 000 segments -- so a twelfth + 64 on top is seven of
    // those; a list beyond it takes k_sampler's own (slow) way.  And as many histogram buckets (a power of two, at
    // least 1 024: a few elements per bucket sort as fast as one) as leave the number of workgroups a CU can hold
    // at its maximum: this kernel is a chain of dependent passes, and chr1's 8 000 segments with 8 192 buckets were
    // 113 KB -- ONE workgroup per CU for the classes that take most of its time (config-4 shape: 22.9 of 27.4 ms)
    const int n0 = (int)P->h_units[(size_t)P->h_order[(size_t)a0]].hist_total;
    const int ccap = std::min<int>(P->h_units[(size_t)P->h_order[(size_t)a0]].slab_cap, (n0 + n0 / 12 + 64 + 63) / 64 * 64);
    auto wgs_at = [&](int nbk_) { return (int)(((size_t)ctx->max_lds) / ((size_t)2 * ccap * 4 + (size_t)(nbk_ + 1) * 4 + 1024)); };
    int cnbk = 8192;
    while (cnbk > 1024 && (cnbk / 2 >= ccap || wgs_at(cnbk) < wgs_at(1024))) cnbk >>= 1;
    size_t lds_k = (size_t)2 * ccap * 4 + (size_t)(cnbk + 1) * 4;
    const int per = (ccap + gat::kMergeThreads - 1) / gat::kMergeThreads;
    const int form = merge_old || per > gat::kMergeRegs ? 0 : (per <= 8 ? 1 : (per <= 16 ? 2 : 3));
    if (form > 0) {
      // (the register forms: the histogram shares the list's LDS -- up to about a bucket per element)
      const int maxb = B.kn.merge_buckets_set ? std::max(1024, (int)B.kn.merge_buckets) : 8192;
      cnbk = 1024;
      while (2 * cnbk + gat::kMergeThreads + 1 <= ccap && 2 * cnbk <= maxb) cnbk <<= 1;     // (+ a word of padding per thread)
      lds_k = ((size_t)ccap + (size_t)std::max(ccap, cnbk + gat::kMergeThreads + 1)) * 4;   // (short lists: the 1 024 buckets and their padding need their own words)
    }
    M.a_base = a0; M.a_end = a1; M.lds_cap = ccap; M.big_buckets = cnbk;
    if (c < GAT_SAMPLER_REPORT_CLASSES) {
      gat_sampler_class_report& rc_ = ctx->sampler_report.cls[c];
      rc_.merge_ccap = ccap; rc_.merge_buckets = cnbk; rc_.merge_form = form == 0 ? 0 : 8 * form;
    }
    hipLaunchKernelGGL(fns[form], grid_yz((unsigned)B.nb, (unsigned)(a1 - a0)), dim3(gat::kMergeThreads), lds_k, call_stream(ctx, P), M);
    HIPCHK(ctx, hipGetLastError());
  }
  A.st2 = P->d_st2.p; A.n_long = (int32_t)n_long;       // (k_sampler reads st2 for those units only)
  if (!B.tail_big) return GAT_OK;
  // the placement rounds behind that consolidation, one stream per lane; k_sampler resumes at the trim
  gat::TailArgs TB;
  TB.S = A;
  TB.cum = nullptr; TB.patch = P->d_patch.p; TB.todo = nullptr; TB.todo_count = nullptr;
  // (counts alone, by k_count_merged -- or through k_contig, which merge(0)s the lists again: what a trim emptied may
  //  stay in the list as [0, 0))
  TB.loose_ok = (B.o.loose_ok && !B.o.need_unit_lists && !B.kn.resume_compact) ? 1 : 0;
  // (bit 0: no bridge between two neighbours, bit 1: none over two segments on the right; "1" or anything else: both off)
  TB.no_bridge = 0;
  if (B.kn.tb_no_bridge_set) { const int v = (int)B.kn.tb_no_bridge; TB.no_bridge = (v == 2 || v == 5) ? (v == 2 ? 2 : 1) : 3; }
  TB.no_log_map = B.kn.tb_no_log_map ? 1 : 0;
  hipLaunchKernelGGL(gat::k_tail_big, grid_yz((unsigned)((B.nb + 63) / 64), n_long), dim3(64), 0, call_stream(ctx, P), TB);
  HIPCHK(ctx, hipGetLastError());
  if (B.resume_big) {
    // ... and the rest of the unit -- log inserted, trim, final filter -- with the list where it is
    // (a reader that takes the segments one by one in any order -- k_count_merged on the units' lists, no contig lists
    //  in between --: the log stays behind the merged list, the trim works on virtual indices)
    const bool virt = TB.loose_ok && !P->merge_contigs && !B.kn.resume_insert;
    ctx->sampler_report.resume_virtual = virt;
    hipLaunchKernelGGL(virt ? gat::k_resume_big<true> : gat::k_resume_big<false>, grid_yz((unsigned)B.nb, n_long), dim3(64), 0, call_stream(ctx, P), TB);
    HIPCHK(ctx, hipGetLastError());
  }
  A.tb = reinterpret_cast<const int32_t*>(P->d_patch.p);
  A.skip_stride = (int32_t)(sizeof(gat::TailPatch) / 4);
  if (B.long_queue) {
    // k_sampler behind them works off a queue: launched over every (sample, unit) -- one or two waves a CU with such
    // lists in LDS -- it took 3.1 ms per 12 500 samples of the config-4 shape to find every unit finished
    TB.todo = P->d_todo.p; TB.todo_count = P->todo_count_dev();
    const int64_t tot = (int64_t)B.nb * B.n_act;
    hipLaunchKernelGGL(gat::k_queue_rest, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, call_stream(ctx, P), TB, (int)B.n_act);
    HIPCHK(ctx, hipGetLastError());
    A.todo = P->d_todo.p; A.todo_count = P->todo_count_dev();
  }
  return GAT_OK;
}

// The split path: first consolidation (k_consolidate, wave per unit), the loop's tail (k_tail, lane per unit), the final list
// (k_finalize, wave per unit) unless the batch's consumer takes (merged list, k_tail's record) -- decided here, for k_contig and
// the count kernels: P->patched_contigs / units_direct / patched_counts.  k_sampler then only resumes -- from the merged list,
// off the queue added to A -- the units k_tail left alone.
static int enqueue_split_path(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, gat::SamplerArgs& A) {
  const int64_t nb = B.nb;
  gat::TailArgs T;
  T.S = A;
  T.loose_ok = 0; T.no_bridge = 0; T.no_log_map = 0;
  T.S.st2 = P->d_st2.p;
  T.S.n_long = (int32_t)(B.merge_big ? B.n_long : 0);         // (the launch positions k_merge_big was given, whose verdict k_consolidate respects)
  T.S.lds_cap = std::min(P->max_unit_cap, 1280);              // k_consolidate: the lists the wave bucket sorts take
  T.S.slab_final = P->d_fslab.p;
  T.cum = P->d_cum.p; T.patch = P->d_patch.p;
  T.todo = P->d_todo.p;
  T.todo_count = P->todo_count_dev();                         // (zeroed with the statistics at the batch's start)
  const size_t lds_max = (size_t)(gat::kSortScratchWords + 2 * (size_t)T.S.lds_cap) * 4;
  // (two kernels: classes whose lists end at 512 segments run the one without the branches -- and registers -- of longer lists)
  void (*const consolidate)(gat::TailArgs) = B.tree ? gat::k_consolidate<true> : gat::k_consolidate<false>;
  void (*const consolidate_long)(gat::TailArgs) = B.tree ? gat::k_consolidate_long<true> : gat::k_consolidate_long<false>;
  HIPCHK(ctx, hipFuncSetAttribute((const void*)consolidate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  HIPCHK(ctx, hipFuncSetAttribute((const void*)consolidate_long, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  // (a call of a few hundred tiles does not fill the chip whatever the LDS of a workgroup: one launch for all classes,
  //  each launch less is a tail less -- config 2 at 1 250 samples: k_consolidate 0.121 -> 0.101 ms)
  const bool one_class = (int64_t)((nb + 63) / 64) * (int64_t)B.n_act <= 1024 && !B.kn.size_classes_set;
  for (size_t c = 0; c + 1 < P->h_class_start.size(); ++c) {
    // one launch per size class, its LDS sized for the class's longest list
    if (one_class && c > 0) break;
    const int a0 = P->h_class_start[c], a1 = one_class ? P->h_class_start.back() : P->h_class_start[c + 1];
    // (as for k_merge_big: LDS for what the class's longest unit is expected to have placed -- its segments +- a renewal
    //  count's spread -- not for its slab region; the rare list beyond it is k_sampler's.  GAT_CONSOLIDATE_SLAB_LDS: the old size)
    const int n0 = (int)P->h_units[(size_t)P->h_order[(size_t)a0]].hist_total;
    const int tight = B.kn.consolidate_slab_lds ? INT32_MAX : (n0 + n0 / 12 + 64 + 31) / 32 * 32;
    const int ccap = std::min(std::min(P->h_units[(size_t)P->h_order[(size_t)a0]].slab_cap, T.S.lds_cap), tight);
    gat::TailArgs C = T;
    C.S.a_base = a0; C.S.a_end = a1; C.S.lds_cap = ccap;
    for (size_t k = c; k + 1 < P->h_class_start.size() && k < GAT_SAMPLER_REPORT_CLASSES && P->h_class_start[k] < a1; ++k)
      ctx->sampler_report.cls[k].consolidate_ccap = ccap;
    const size_t lds_c = (size_t)(gat::kSortScratchWords + 2 * (size_t)ccap) * 4;
    hipLaunchKernelGGL(ccap > 512 ? consolidate_long : consolidate, grid_yz((unsigned)nb, (unsigned)(a1 - a0)), dim3(64), lds_c, call_stream(ctx, P), C);
    HIPCHK(ctx, hipGetLastError());
  }
  if (B.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k[2], call_stream(ctx, P)));
  const bool long_ws = P->tail_long_ws && P->max_nws > gat::kTailMaxWs;
  hipLaunchKernelGGL(long_ws ? gat::k_tail<true> : gat::k_tail<false>, grid_yz((unsigned)((nb + 63) / 64), B.n_act), dim3(64), 0, call_stream(ctx, P), T);
  HIPCHK(ctx, hipGetLastError());
  if (B.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_t[0], call_stream(ctx, P)));
  // isochore problems: k_contig re-sorts the units of a contig anyway and takes (merged list, k_tail's record) as
  // it is -- no final unit lists unless somebody asked for them (gat_sample_units)
  P->patched_contigs = P->merge_contigs && P->n_contigs > 0 && !B.o.need_unit_lists && !B.kn.contig_final_lists;
  P->units_direct = B.o.units_direct && P->patched_contigs && P->units_direct_ok && B.o.serial_state == nullptr;
  P->patched_counts = !P->merge_contigs && B.o.records_ok && !B.o.need_unit_lists;
  if (!P->patched_contigs && !P->patched_counts) hipLaunchKernelGGL(gat::k_finalize, grid_yz((unsigned)nb, B.n_act), dim3(64), 0, call_stream(ctx, P), T);
  HIPCHK(ctx, hipGetLastError());
  if (B.timed) { HIPCHK(ctx, hipEventRecord(ctx->ev_t[1], call_stream(ctx, P))); ctx->t_recorded = true; }
  A.st2 = P->d_st2.p; A.n_long = (int32_t)B.n_act;
  A.slab_final = P->d_fslab.p;
  A.skip = &P->d_patch.p->state;
  A.skip_stride = (int32_t)(sizeof(gat::TailPatch) / 4);
  A.todo = P->d_todo.p; A.todo_count = P->todo_count_dev();
  return GAT_OK;
}

// k_sampler / k_serial by variant: sampler kind x (long lists: counting-sort scratch) x (workspaces beyond the register loop:
// search trees) -- 0..3 SamplerAnnotator, 4 / 5 SamplerSegments, 6 / 7 lists beyond LDS -- and 8, k_sampler's alone: variant 0
// with registers for 5 waves per SIMD
typedef void (*sampler_fn)(gat::SamplerArgs);
static const sampler_fn kSamplerFns[9] = {
    gat::k_sampler<0, false, false, false>, gat::k_sampler<0, false, true, false>, gat::k_sampler<0, true, false, false>,
    gat::k_sampler<0, true, true, false>, gat::k_sampler<1, false, false, false>, gat::k_sampler<1, false, true, false>,
    gat::k_sampler<0, false, false, true>, gat::k_sampler<0, false, true, true>, gat::k_sampler<0, false, false, false, 5>};
static const sampler_fn kSerialFns[8] = {
    gat::k_serial<0, false, false, false>, gat::k_serial<0, false, true, false>, gat::k_serial<0, true, false, false>,
    gat::k_serial<0, true, true, false>, gat::k_serial<1, false, false, false>, gat::k_serial<1, false, true, false>,
    gat::k_serial<0, false, false, true>, gat::k_serial<0, false, true, true>};
// the enqueue function of a list sampler (gat_samplers.h: wave_per_unit) by sampler id; SamplerAnnotator / SamplerSegments have
// none: enqueue_placement_sampler
typedef int (*list_enqueue_fn)(gat_ctx*, gat_problem*, const BatchPlan&, uint32_t, int64_t);
static const struct ListEnqueueFns {
  list_enqueue_fn fn[kNumSamplers] = {};
  constexpr ListEnqueueFns() {
    fn[GAT_SAMPLER_SHIFT] = enqueue_shift;
    fn[GAT_SAMPLER_GLOBAL_PERMUTATION] = enqueue_permute;
    fn[GAT_SAMPLER_LOCAL_PERMUTATION] = enqueue_permute_local;
    fn[GAT_SAMPLER_BRUTE_FORCE] = enqueue_brute_force;
    fn[GAT_SAMPLER_CIRCULAR] = enqueue_circular;
    fn[GAT_SAMPLER_UNIVERSE] = enqueue_universe;
  }
} kListEnqueueFns;

// k_sampler over what the stages in front of it left it (everything, without them) -- or k_serial: the reference's own stream
static int enqueue_sampler(gat_ctx* ctx, const gat_problem* P, const BatchPlan& B, const gat::SamplerArgs& A) {
  const int64_t nb = B.nb;
  int variant = P->sampler == GAT_SAMPLER_SEGMENTS ? (B.tree ? 5 : 4)
              : B.huge ? (B.tree ? 7 : 6) : (B.long_lists ? 2 : 0) + (B.tree ? 1 : 0);
  // short lists only (20 waves of this kernel fit a CU's LDS): the instantiation with registers for 5 waves per SIMD
  if (variant == 0 && (int64_t)B.lds * 20 <= ctx->max_lds && !B.kn.no_wpe5) variant = 8;
  ctx->sampler_report.sampler_variant = variant;
  HIPCHK(ctx, hipFuncSetAttribute((const void*)kSamplerFns[variant], hipFuncAttributeMaxDynamicSharedMemorySize, (int)B.lds));
  auto launch_sampler = [&](const dim3& gs, size_t lds_, const gat::SamplerArgs& K) {
    hipLaunchKernelGGL(kSamplerFns[variant], gs, dim3(64), lds_, call_stream(ctx, P), K);
  };
  const dim3 off_queue((unsigned)std::min<int64_t>((int64_t)nb * B.n_act, 8192));
  const bool list_in_lds = !B.huge && P->sampler != GAT_SAMPLER_SEGMENTS;
  if (B.o.serial_state != nullptr) {
    // the reference's own stream: one wave, every (sample, unit) of the batch in order
    gat::SamplerArgs K = A;
    K.serial_state = B.o.serial_state; K.unit_pos = P->d_unit_pos.p;
    const sampler_fn serial = kSerialFns[variant == 8 ? 0 : variant];
    HIPCHK(ctx, hipFuncSetAttribute((const void*)serial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)B.lds));
    hipLaunchKernelGGL(serial, dim3(1), dim3(64), B.lds, call_stream(ctx, P), K);
  } else if (B.split) {
    launch_sampler(off_queue, B.lds, A);
  } else if (list_in_lds && A.big_buckets == 0 && P->h_class_start.size() > 2 &&
             !(A.todo_count != nullptr && P->max_nws <= gat::kWsTreeMin && !B.kn.size_classes_set)) {
    // (not behind k_resume_big where it takes every unit -- workspaces of up to 32 segments --: the queue then holds the
    //  per cent of units it declined, and one launch runs them side by side where five ran them class after class)
    // one launch per size class: LDS for the class's longest list
    for (size_t c = 0; c + 1 < P->h_class_start.size(); ++c) {
      const int a0 = P->h_class_start[c], a1 = P->h_class_start[c + 1];
      const int ccap = P->h_units[(size_t)P->h_order[(size_t)a0]].slab_cap;
      gat::SamplerArgs K = A;
      K.a_base = a0; K.a_end = a1;
      const unsigned cnt = (unsigned)(a1 - a0);
      // (off the queue -- long lists behind k_resume_big --: a one-dimensional launch, every class takes its own entries)
      const dim3 gc = A.todo_count != nullptr ? dim3((unsigned)std::min<int64_t>((int64_t)nb * cnt, 8192)) : grid_yz((unsigned)nb, cnt);   // (8 192: what is left is a few long units, one to a workgroup)
      launch_sampler(gc, (size_t)(gat::kMtLdsWords + 2 * (size_t)ccap) * 4, K);
    }
  } else if (A.todo_count != nullptr) {
    launch_sampler(off_queue, B.lds, A);
  } else {
    launch_sampler(grid_yz((unsigned)nb, B.n_act), B.lds, A);
  }
  HIPCHK(ctx, hipGetLastError());
  return GAT_OK;
}

// SamplerAnnotator / SamplerSegments: the stages the plan names in front of k_sampler, then k_sampler (or k_serial).  A is left
// as k_sampler saw it: k_reduce_stats reads from it which units k_tail finished / k_tail_big carried on.
static int enqueue_placement_sampler(gat_ctx* ctx, gat_problem* P, const BatchPlan& B, uint32_t seed, int64_t begin, gat::SamplerArgs& A) {
  int rc = base_sampler_args(ctx, P, B, seed, begin, A);
  if (!rc && B.smode) rc = enqueue_front_end(ctx, P, B, A);
  if (rc) return rc;
  ctx->k_recorded = B.timed && B.smode;
  A.lds_cap = P->max_unit_cap;           // (the list kernels' fields: the front end reads neither)
  A.big_buckets = B.big_buckets;
  if (B.merge_big && (rc = enqueue_long_lists(ctx, P, B, A))) return rc;
  P->split_ran = B.split;
  if (B.split) rc = enqueue_split_path(ctx, P, B, A);
  else if (B.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k[2], call_stream(ctx, P)));
  if (!rc) rc = enqueue_sampler(ctx, P, B, A);
  if (rc) return rc;
  if (B.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k[3], call_stream(ctx, P)));
  return GAT_OK;
}

// fromIsochores: the units' lists of a contig united into the contig's list (k_contig<HUGE, NOSORT>), one launch per size class
typedef void (*contig_fn)(gat::ContigArgs);
static const contig_fn kContigFns[2][2] = {{gat::k_contig<false>, gat::k_contig<true>},                 // [nosort][huge]
                                           {gat::k_contig<false, true>, gat::k_contig<true, true>}};
static int enqueue_contigs(gat_ctx* ctx, gat_problem* P, const Knobs& kn, int64_t nb) {
  gat::ContigArgs B;
  B.contig_unit_off = P->d_contig_unit_off.p; B.contig_units = P->d_contig_units.p; B.units = P->d_units.p;
  B.cu_rec = P->d_cu_rec.p;
  B.contig_slab_off = P->d_contig_slab_off.p; B.n_units = P->n_units; B.n_contigs = P->n_contigs;
  B.slab_in = P->final_slab(); B.slab_out = P->d_cslab.p; B.slab_stride = P->slab_stride;
  B.unit_n = P->d_unit_n.p; B.contig_n = P->d_contig_n.p; B.stat = P->d_stat.p;
  B.slab_merged = nullptr; B.unit_pos = P->d_unit_pos.p; B.st2 = nullptr; B.patch = nullptr; B.patch_stride = 0;
  B.ws_stat = P->d_ws_stat.p;
  B.rec_stride = (int32_t)P->batch;
  if (P->split_ran && P->patched_contigs) {
    B.slab_merged = P->d_slab.p;
    B.st2 = P->d_st2.p;
    B.patch = reinterpret_cast<const int32_t*>(P->d_patch.p);
    B.patch_stride = (int32_t)(sizeof(gat::TailPatch) / 4);
  }
  const int need_max = P->h_contig_order.empty() ? 64 : P->h_contig_need[(size_t)P->h_contig_order[0]];
  size_t lds = (size_t)std::max(64, need_max) * 8 + gat::kSortScratchWords * 4;
  const bool huge_c = (int64_t)lds > ctx->max_lds || kn.test_huge;   // list stays in the output slab
  if (huge_c) lds = gat::kSortScratchWords * 4;
  // (units_direct: the lists only concatenated, the candidates for k_units_overlap noted: k_contig<., true>)
  const bool nosort = P->units_direct;
  B.bmap = P->d_bmap.p; B.bmap_off = P->d_bmap_off.p; B.bshift = P->bshift;
  B.cand = P->d_cand.p; B.cand_cap = (uint32_t)(P->d_cand.n / gat::kCandSlots); B.cand_count = P->d_cand_count.p;
  const contig_fn kc = kContigFns[nosort ? 1 : 0][huge_c ? 1 : 0];
  HIPCHK(ctx, hipFuncSetAttribute((const void*)kc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  B.order = P->d_contig_order.p;
  B.flags = P->flags_dev();
  // one launch per size class: LDS for the class's longest expected list (more waves per CU for the short contigs)
  for (size_t k = 0; k + 1 < P->h_contig_class_start.size(); ++k) {
    const int c0 = P->h_contig_class_start[k], c1 = P->h_contig_class_start[k + 1];
    // (one launch where the list is put together in place: beyond LDS, or only concatenated)
    const bool one = huge_c || nosort;
    if (one && k > 0) break;
    B.base = one ? 0 : c0;
    B.count = one ? P->n_contigs : c1 - c0;
    B.lds_cap = one ? 0 : std::max(64, P->h_contig_need[(size_t)P->h_contig_order[(size_t)c0]]);
    const size_t lds_k = nosort ? 64 : (huge_c ? lds : (size_t)B.lds_cap * 8 + gat::kSortScratchWords * 4);
    hipLaunchKernelGGL(kc, grid_yz((unsigned)nb, (unsigned)B.count), dim3(64), lds_k, call_stream(ctx, P), B);
    HIPCHK(ctx, hipGetLastError());
  }
  return GAT_OK;
}

// ---- a sampler batch whose kernels have completed (the stream has been synchronised): its checks, then its statistics ----
// a batch that did not fit: the slab laid out again (the caller has set what the new layout takes), the batch to be repeated
static int relayout_and_repeat(gat_ctx* ctx, gat_problem* P, const Knobs& kn, int64_t nb, gat_stats* st, const char* too_large) {
  if (layout_slab(P, kn)) return set_err(ctx, GAT_ERR_CAPACITY, "%s", too_large);
  if (const int rc = upload_layout(ctx, P, kn)) return rc;
  if (st) st->n_retried += nb * (int64_t)P->h_order.size();
  return kRelayout;
}

// The status checks: an error, kRelayout (nothing of the batch is valid: the caller repeats it), or GAT_OK.  The statistics that go
// with a check -- SamplerBruteForce's, k_units_overlap's -- are added here: a call that fails on them still reports them
static int check_batch_status(gat_ctx* ctx, gat_problem* P, const Knobs& kn, int64_t nb, gat_stats* st, const unsigned long long* h_stat) {
  const int32_t flags = *reinterpret_cast<const int32_t*>(h_stat + gat::kStatFlags);
  if (flags & gat::kStatusCoordRange)
    return set_err(ctx, GAT_ERR_ASSERT, "SamplerLocalPermutation: a sampled coordinate exceeds 2^31 - 1 before it wraps (flags=%d): the reference "
                                        "raises OverflowError (gat/Engine.pyx:1208, :1212)", flags);
  if (flags & (gat::kStatusAssert | gat::kStatusTrimAssert))
    return set_err(ctx, GAT_ERR_ASSERT, "sampler assertion failed on device (flags=%d): %s", flags,
                   (flags & gat::kStatusAssert) ? "sampled list has no overlap with the workspace (gat/Engine.pyx:645)"
                                                : "trimming more than the total length (gat/SegmentList.pyx:560)");
  if ((flags & gat::kStatusContigLds) && !(flags & gat::kStatusOverflow)) {
    // a contig's lists were longer than expected: LDS for every unit at its capacity from now on, batch repeated
    P->contig_tight = false;
    return relayout_and_repeat(ctx, P, kn, nb, st, "per-sample slab exceeds 2^31 segments");
  }
  if (flags & gat::kStatusOverflow) {
    // (doubled until the lists fit: a unit whose segments are longer than its whole workspace beside one of a few bases places
    //  thousands of the small one between the large one's trims -- two of 200 000 edge-case seeds needed more than 64 x 128 slots,
    //  which the reference's lists simply grow to (round 6); the per-sample slab's 2^31 segments and the device's memory end it)
    if (P->cap_scale >= (1 << 20)) return set_err(ctx, GAT_ERR_CAPACITY, "sampler slab overflow even at 2^20 x capacity");
    P->cap_scale *= 2;
    return relayout_and_repeat(ctx, P, kn, nb, st, "per-sample slab exceeds 2^31 segments after growth");
  }
  if (P->sampler == GAT_SAMPLER_BRUTE_FORCE) {
    // (behind the overflow check: a batch that is repeated is counted once, as it stands in the end)
    const unsigned long long restarts = h_stat[gat::kStatRestarts];
    const int64_t unconv = (int64_t)(restarts >> gat::kBruteUnconvShift);
    if (st) { st->n_restarts += (int64_t)(restarts & ((1ull << gat::kBruteUnconvShift) - 1ull)); st->n_unconverged += unconv; }
    if (unconv) {
      const unsigned long long first = ~h_stat[gat::kStatBruteFirst];
      return set_err(ctx, GAT_ERR_VALUE, "SamplerBruteForce: sampling did not converge: sample %lld, unit %d used up its %d passes of %d tries "
                                         "(%lld work units of the batch; gat/Engine.pyx:868-869)", (long long)(first >> 32), (int)(first & 0xffffffffull),
                     (int)P->brute_ntries_outer, (int)P->brute_ntries_inner, (long long)unconv);
    }
  }
  // k_units_overlap: overlaps between the units' lists that were not pairwise, or more candidates than the buffer holds --
  // the batch is repeated through k_contig, and the problem keeps to that
  const uint32_t* uw = reinterpret_cast<const uint32_t*>(h_stat + gat::kStatUnitsOverlap);
  if (P->units_direct && P->units_direct_ok && uw[0] != 0u) {
    if ((uw[0] & 1u) != 0u || P->cand_scale >= 64) P->units_direct_ok = false;   // not pairwise (or a buffer that will not do)
    else P->cand_scale *= 4;                                                       // a candidate region was too small
    if (st) st->n_retried += nb * (int64_t)P->h_order.size();
    return kRelayout;
  }
  if (st && P->units_direct) { st->n_straddle_candidates += (int64_t)uw[2]; st->n_unit_overlaps += (int64_t)uw[1]; }
  return GAT_OK;
}

#if defined(GAT_DIAG) || defined(GAT_DIAG_CONS)
// diagnostic builds: what the kernels noted about the batch, appended to the file GAT_DIAG_OUT names
static int dump_batch_diag(gat_ctx* ctx, gat_problem* P, const Knobs& kn, int64_t nb) {
  if (const char* fn = kn.diag_out.empty() ? nullptr : kn.diag_out.c_str()) {
    // shares of a k_sampler work unit's life per phase, summed over the batch (tools/diag_sampler.sh)
    const size_t nd = (size_t)nb * std::max(1, P->n_units) * 8;
    std::vector<unsigned long long> h(nd);
    HIPCHK(ctx, staged_d2h(ctx, h.data(), P->d_diag.p, nd * 8));
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < nd; ++i) sum[i & 7] += (double)h[i];
    if (FILE* f = fopen(fn, "a")) {
      fprintf(f, "{\"work_units\": %lld, \"cycles\": {\"prologue\": %.0f, \"sort\": %.0f, \"merge\": %.0f, \"coverage\": %.0f, "
                 "\"fast_paths\": %.0f, \"trim\": %.0f, \"draws_placement\": %.0f, \"final_filter_write\": %.0f}}\n",
              (long long)nb * (long long)P->h_order.size(), sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], sum[7]);
      if (P->d_diag_place.n >= P->h_order.size() * 8 && !P->h_order.empty()) {
        // k_place's loop, per phase: over all tiles, and for the largest unit alone (launch position 0: the tile the kernel ends with)
        std::vector<unsigned long long> hp(P->h_order.size() * 8);
        if (staged_d2h(ctx, hp.data(), P->d_diag_place.p, hp.size() * 8) == hipSuccess) {
          double all[7] = {0, 0, 0, 0, 0, 0, 0};
          for (size_t i = 0; i < hp.size(); ++i) all[i & 7] += (i & 7) < 7 ? (double)hp[i] : 0.0;
          fprintf(f, "{\"k_place\": {\"all_tiles\": {\"row_wait\": %.0f, \"lookups\": %.0f, \"steps\": %.0f, \"flush\": %.0f, \"loop_control\": %.0f, "
                     "\"rows\": %.0f, \"tiles\": %.0f}, \"largest_unit\": {\"row_wait\": %llu, \"lookups\": %llu, \"steps\": %llu, \"flush\": %llu, "
                     "\"loop_control\": %llu, \"rows\": %llu, \"tiles\": %llu}}}\n",
                  all[0], all[1], all[2], all[3], all[4], all[5], all[6], hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6]);
        }
      }
      {
        // k_place's hand-over records by kind: pending length (triggered), -1 run in full, -2 complete, -3 resume
        const size_t n_act = P->h_order.size();
        std::vector<int4> hs(n_act * (size_t)P->batch);
        if (n_act && P->d_st.n >= hs.size() && staged_d2h(ctx, hs.data(), P->d_st.p, hs.size() * sizeof(int4)) == hipSuccess) {
          long long kinds[5] = {0, 0, 0, 0, 0};
          int shown = 0;
          fprintf(f, "{\"k_place_handover_examples\": [");
          for (size_t a = 0; a < n_act; ++a)
            for (int64_t i = 0; i < nb; ++i) {
              const int4 r = hs[a * (size_t)P->batch + (size_t)i];
              kinds[r.z > 0 ? 0 : (r.z == -1 ? 1 : (r.z == -2 ? 2 : (r.z == -3 ? 3 : 4)))]++;
              if (r.z <= 0 && shown < 12) fprintf(f, "%s[%zu, %lld, %d, %d, %d, %d, %d]", shown++ ? ", " : "", a, (long long)i, r.x, r.y, r.z, r.w, P->h_rng_rows.empty() ? -1 : P->h_rng_rows[a]);
            }
          {
            long long sx = 0, sy = 0, sz = 0, sw = 0;
            for (size_t a = 0; a < n_act; ++a) for (int64_t i = 0; i < nb; ++i) { const int4 r = hs[a * (size_t)P->batch + (size_t)i]; sx += r.x; sy += r.y; sz += r.z; sw += r.w; }
            fprintf(f, "], \"k_place_handover_sums\": [%lld, %lld, %lld, %lld", sx, sy, sz, sw);
          }
          fprintf(f, "], \"k_place_handover\": {\"triggered\": %lld, \"in_full\": %lld, \"complete\": %lld, \"resume\": %lld, \"other\": %lld}}\n",
                  kinds[0], kinds[1], kinds[2], kinds[3], kinds[4]);
        }
      }
      {
        // k_place's tiles in time: per unit (launch position) the first begin, the median begin, the median and the last end of
        // its tiles, in microseconds from the kernel's first begin
        const size_t n_act = P->h_order.size(), ntl = (size_t)((nb + 63) / 64);
        std::vector<unsigned long long> ht(n_act * ntl * 2);
        if (n_act && ntl && P->d_diag_tiles.n >= ht.size() && staged_d2h(ctx, ht.data(), P->d_diag_tiles.p, ht.size() * 8) == hipSuccess) {
          unsigned long long t_min = ~0ull;
          for (size_t i = 0; i < ht.size(); i += 2) if (ht[i] && ht[i] < t_min) t_min = ht[i];
          fprintf(f, "{\"k_place_tiles\": [");
          for (size_t a = 0; a < n_act; ++a) {
            std::vector<double> b0, e0;
            for (size_t t = 0; t < ntl; ++t) {
              const unsigned long long x = ht[(a * ntl + t) * 2], y = ht[(a * ntl + t) * 2 + 1];
              if (x && y) { b0.push_back((double)(x - t_min) / 100.0); e0.push_back((double)(y - t_min) / 100.0); }
            }
            if (b0.empty()) continue;
            std::sort(b0.begin(), b0.end()); std::sort(e0.begin(), e0.end());
            fprintf(f, "%s{\"a\": %zu, \"segments\": %u, \"tiles\": %zu, \"begin_first\": %.1f, \"begin_median\": %.1f, \"begin_last\": %.1f, "
                       "\"end_first\": %.1f, \"end_median\": %.1f, \"end_last\": %.1f}", a ? ", " : "", a,
                    P->h_units[(size_t)P->h_order[a]].hist_total, b0.size(), b0.front(), b0[b0.size() / 2], b0.back(), e0.front(), e0[e0.size() / 2], e0.back());
          }
          fprintf(f, "]}\n");
        }
      }
      fclose(f);
    }
  }
  return GAT_OK;
}
#endif

// the batch's statistics words and, in a timed call, its event laps into the caller's gat_stats
static void add_batch_stats(gat_ctx* ctx, const gat_problem* P, gat_stats* st, bool timed, const unsigned long long* h_stat) {
  st->n_placed += (int64_t)h_stat[gat::kStatPlaced];
  st->n_draws += (int64_t)h_stat[gat::kStatDraws];
  st->n_unsuccessful += (int64_t)h_stat[gat::kStatUnsuccessful];
  st->n_tail_units += (int64_t)h_stat[gat::kStatTailUnits];
  if (P->split_ran && (P->patched_contigs || P->patched_counts)) st->lists_from_records += 1;
  st->n_full_units += (int64_t)h_stat[gat::kStatFullUnits];
  st->n_resumed_units += (int64_t)h_stat[gat::kStatResumedUnits];
  st->n_queued_units += (int64_t)(h_stat[gat::kStatQueued] & 0xffffffffull);
  st->n_empty_windows += (int64_t)h_stat[gat::kStatEmptyWindows];
  if (timed) {
    // (a timing query that fails leaves its figure at 0: it must not turn a call that computed its counts into an error)
    auto lap = [](hipEvent_t a, hipEvent_t b) { float ms = 0; if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); ms = 0; } return ms; };
    st->ms_sampler += lap(ctx->ev[0], ctx->ev[1]);
    st->ms_contig += lap(ctx->ev[1], ctx->ev[2]);
    if (ctx->k_recorded && !P->h_order.empty()) {
      st->ms_rng += lap(ctx->ev[0], ctx->ev_k[0]);
      st->ms_place += lap(ctx->ev_k[0], ctx->ev_k[1]);
      st->ms_merge += lap(ctx->ev_k[1], ctx->ev_k[2]);
      st->ms_tail += lap(ctx->ev_k[2], ctx->ev_k[3]);
      if (ctx->t_recorded) {
        st->ms_ktail += lap(ctx->ev_k[2], ctx->ev_t[0]);
        st->ms_finalize += lap(ctx->ev_t[0], ctx->ev_t[1]);
      }
    }
  }
}

static int finish_sampler_batch(gat_ctx* ctx, gat_problem* P, const Knobs& kn, int64_t nb, gat_stats* st, bool timed, const unsigned long long* h_stat) {
  int rc = check_batch_status(ctx, P, kn, nb, st, h_stat);
#if defined(GAT_DIAG) || defined(GAT_DIAG_CONS)
  if (!rc) rc = dump_batch_diag(ctx, P, kn, nb);
#endif
  if (!rc && st) add_batch_stats(ctx, P, st, timed, h_stat);
  return rc;
}

// One batch as the sequence of its stages: scratch and statistics reset, the units' sampler, fromIsochores, the statistics and
// -- unless deferred -- the synchronisation and the batch's checks.
static int run_sampler_batch(gat_ctx* ctx, gat_problem* P, const Knobs& kn, uint32_t seed, int64_t begin, int64_t nb,
                             gat_stats* st, bool timed, const BatchOpts& o = BatchOpts()) {
  unsigned long long* h_stat = o.h_stat != nullptr ? o.h_stat : ctx->h_stat;
  P->units_direct = false;
  int rc = ensure_scratch(ctx, P, kn, nb);
  if (rc) return rc;
  if (P->batch < nb) return set_err(ctx, GAT_ERR_MEMORY, "internal: batch %lld > scratch %lld", (long long)nb, (long long)P->batch);
  // (unit_n, contig_n and ws_stat are zeroed once when allocated: the kernels rewrite every entry of the active units
  //  in every batch and never touch the others)
#ifdef GAT_DBG_QUEUE
  HIPCHK(ctx, hipMemsetAsync(P->d_stat.p, 0, gat::kStatSlotWords * 8, call_stream(ctx, P)));     // (kStatDbgWhy too)
#else
  HIPCHK(ctx, hipMemsetAsync(P->d_stat.p, 0, gat::kStatCopied * 8, call_stream(ctx, P)));
#endif
  if (o.units_direct && P->d_cand_count.n) HIPCHK(ctx, hipMemsetAsync(P->d_cand_count.p, 0, P->d_cand_count.n * 4, call_stream(ctx, P)));
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev[0], call_stream(ctx, P)));
  gat::SamplerArgs A = {};                 // (SamplerAnnotator / SamplerSegments: what k_sampler saw)
  if (!P->h_order.empty()) {
    // (what a stage records or leaves in place of final lists, it says itself)
    if (timed) ctx->k_recorded = ctx->t_recorded = false;     // (the timed call's: another problem's call beside it leaves them)
    P->split_ran = P->patched_contigs = P->patched_counts = false;
    const BatchPlan B = plan_batch(ctx, kn, P, nb, timed, o);
    record_plan(ctx, P, B);
    const list_enqueue_fn enqueue_list = kListEnqueueFns.fn[P->sampler];     // (a problem's sampler is a known one: gat_problem_create)
    if (enqueue_list != nullptr && o.serial_state != nullptr)
      return set_err(ctx, GAT_ERR_ARG, "%s has no reference-stream mode", sampler_info(P->sampler)->name);
    rc = enqueue_list != nullptr ? enqueue_list(ctx, P, B, seed, begin) : enqueue_placement_sampler(ctx, P, B, seed, begin, A);
    if (rc) return rc;
  }
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev[1], call_stream(ctx, P)));
  if (P->merge_contigs && P->n_contigs > 0 && (rc = enqueue_contigs(ctx, P, kn, nb))) return rc;
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev[2], call_stream(ctx, P)));
  if (!P->h_order.empty()) {
    // (behind k_contig: on isochore problems it is k_contig that writes the statistics of the units k_tail finished)
    const int32_t* skip_ptr = A.skip != nullptr ? A.skip : A.tb;     // (n_tail_units: finished by k_tail / carried on by k_tail_big)
    hipLaunchKernelGGL(gat::k_reduce_stats, dim3(256), dim3(256), 0, call_stream(ctx, P), (const uint32_t*)P->d_ws_stat.p,
                       (int64_t)nb, (int64_t)P->n_units, (int64_t)P->batch, P->d_stat.p, skip_ptr, A.skip_stride);
    HIPCHK(ctx, hipGetLastError());
  }
#ifdef GAT_DBG_QUEUE
  { unsigned long long w[gat::kStatSlotWords]; hipStreamSynchronize(call_stream(ctx, P)); hipMemcpy(w, P->d_stat.p, sizeof(w), hipMemcpyDeviceToHost);
    const unsigned long long* why = w + gat::kStatDbgWhy;          // (kStatDbgWhyWords = 6 of them)
    fprintf(stderr, "round broken by: empty segment %llu, placeholder neighbour %llu, both neighbours and more %llu, two on the right %llu, two logged %llu, logged + neighbour %llu\n", why[0], why[1], why[2], why[3], why[4], why[5]); }
#endif
  HIPCHK(ctx, hipMemcpyAsync(h_stat, P->d_stat.p, gat::kStatCopied * 8, hipMemcpyDeviceToHost, call_stream(ctx, P)));
  if (P->sampler == GAT_SAMPLER_BRUTE_FORCE)
    HIPCHK(ctx, hipMemcpyAsync(h_stat + gat::kStatBruteFirst, P->d_stat.p + gat::kStatBruteFirst, 8, hipMemcpyDeviceToHost, call_stream(ctx, P)));
  if (o.defer) return GAT_OK;
  HIPCHK(ctx, hipStreamSynchronize(call_stream(ctx, P)));
  return finish_sampler_batch(ctx, P, kn, nb, st, timed, h_stat);
}

static void fill_count_args(gat_problem* P, gat::CountArgs& A, int64_t nb) {
  A.seg = P->merge_contigs ? P->d_cslab.p : P->final_slab();
  A.seg_stride = P->slab_stride;
  A.c_off = P->d_count_c_off.p;
  A.n_arr = P->merge_contigs ? P->d_contig_n.p : P->d_unit_n.p;
  A.n_stride = P->merge_contigs ? P->n_contigs : P->n_units;
  A.n_index = P->d_count_n_index.p;
  A.cws_nseg = P->d_cws_nseg.p;
  A.n_contigs = P->n_contigs;
  A.n_tracks = P->n_tracks;
  A.n_samples = (int32_t)nb;
  if (P->split_ran && P->units_direct) {       // k_contig only concatenated: k_units_overlap mends (it reads the units' lists themselves)
    A.contig_unit_off = P->d_contig_unit_off.p;
    A.cu_rec = P->d_cu_rec.p;
    A.unit_n = P->d_unit_n.p;
    A.seg_units = P->final_slab();
    A.seg_units_merged = P->d_slab.p;
    A.cand = P->d_cand.p; A.cand_cap = (uint32_t)(P->d_cand.n / gat::kCandSlots);
    A.cand_count = P->d_cand_count.p;
  }
  if (P->split_ran && P->patched_counts) {     // no k_finalize ran: k_count_seg<.., PATCH> reads merged lists + records
    A.seg_merged = P->d_slab.p;
    A.unit_pos = P->d_unit_pos.p;
  }
  if (P->split_ran && (P->units_direct || P->patched_counts)) {     // (either way: k_merge_big's and k_tail's records)
    A.st2 = P->d_st2.p;
    A.patch = reinterpret_cast<const int32_t*>(P->d_patch.p);
    A.patch_stride = (int32_t)(sizeof(gat::TailPatch) / 4);
    A.n_units = P->n_units;
    A.rec_stride = (int32_t)P->batch;
  }
}

// ---- the batch seam: enqueue / wait ---------------------------------------------------------------------------
// A call is cut into batches that fit the scratch budget.  call_begin enqueues them one behind the other on the call's
// stream (call_stream: the context's, or -- with another problem's call in flight -- one of its lanes, call_lane_for:
// the fork in front of the first count kernel, the join behind the enqueue) -- sampler kernels, count kernels, the copy of the batch's status word and statistics into a pinned slot of its own
// -- up to kMaxInflight of them, and returns; the host does what else it has to do.  call_wait synchronises once, reads the
// slots in order, and where a batch has to be repeated (a unit's region overflowed, a contig's lists beyond the launch's
// LDS) lays the slab out again and enqueues that batch and everything behind it once more: results do not depend on the
// batching (streams are per unit) and every batch writes its own columns of the count matrix.
// sample lists much longer than the annotation lists they meet: swap the roles in the count kernel (needs the tables' size)
static void decide_swap(gat_problem* P) {
  if (P->swap_decided) return;
  P->swap_decided = true;
  const int64_t total = annotations_ready(P->anno) ? P->anno->dev.total : P->anno->total_known;   // (callers: ready, or total_known >= 0)
  const double avg_n = P->n_contigs ? (double)P->n_seg_total / P->n_contigs : 0.0;
  const double avg_m = (P->n_contigs && P->n_tracks) ? (double)total / ((double)P->n_contigs * P->n_tracks) : 0.0;
  if (avg_m > 0 && avg_n > 3.0 * avg_m) P->swap_capx = 1;       // capacity is taken from the slab layout at launch
}

static int call_swap_capx(const gat_ctx* ctx, const gat_problem* P) {
  if (!P->swap_capx) return 0;
  const int capx = P->merge_contigs ? P->max_contig_cap : P->max_unit_cap;
  return ((int64_t)3 * capx * 4 + (8192 + 1) * 4 <= (int64_t)ctx->max_lds - 1024) ? capx : 0;
}

// (the stages call_enqueue_more schedules)  The count kernels of the newest batch (the tables are there, or are waited for), behind them k_units_overlap's words into the
// batch's slot and -- behind the call's last batch -- the call's end
static int enqueue_count_stage(gat_ctx* ctx, gat_problem* P, const Counters& C) {
  CallState& K = P->call;
  int rc = annotations_wait(ctx, P->anno);
  if (rc) return rc;
  decide_swap(P);
  const int slot = K.n_flight - 1;
  const int64_t nb = K.nb[slot];
  const int swap_capx = call_swap_capx(ctx, P);
  K.mstat_on = P->anno->dev.has_merged;
  if (K.lane >= 0 && !K.fork_waited) {
    // the fork: the count kernels are the call's first access to memory of the caller's (the count matrix) -- what the
    // caller ordered in front of the call on its stream is in front of them.  The sampler kernels before this point
    // touch the problem's own scratch and the read-only tables alone and started without waiting
    HIPCHK(ctx, hipStreamWaitEvent(call_stream(ctx, P), K.blk->ev_fork, 0));
    K.fork_waited = true;
  }
  if (K.mstat_on && K.enq == nb) {
    // (k_count_merged's own traffic counters: only a problem with a merged index can take that kernel; zeroed in front of
    //  the call's first count kernel)
    if (P->d_mstat.n < 512) HIPCHK(ctx, P->d_mstat.alloc(512));
    HIPCHK(ctx, hipMemsetAsync(P->d_mstat.p, 0, 512 * 8, call_stream(ctx, P)));
  }
  gat::CountArgs A;
  memset(&A, 0, sizeof(A));
  fill_count_args(P, A, nb);
  A.out = (int64_t*)K.counts_dev; A.out_stride = K.S; A.out_begin = K.enq - nb;
  A.mstat = K.mstat_on ? P->d_mstat.p : nullptr;
  if (K.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_cnt[0], call_stream(ctx, P)));
  CountLaunch L;
  L.stream = call_stream(ctx, P); L.ev_main = K.blk->ev_main[slot];
  L.units = P->d_units.p; L.ws = P->d_ws.p; L.ws_tree = P->d_ws_tree.p;
  for (int c = 0; c < P->n_contigs; ++c) L.max_units = std::max(L.max_units, P->h_contig_unit_off[(size_t)c + 1] - P->h_contig_unit_off[(size_t)c]);
  if ((rc = launch_count(ctx, K.knobs, P->anno->dev, C, A, P->d_part, swap_capx,
                         P->merge_contigs ? P->max_contig_cap : P->max_unit_cap, L))) return rc;
  unsigned long long* uo = K.blk->stat_slot(slot) + gat::kStatUnitsOverlap;
  if (A.cu_rec != nullptr)       // (k_units_overlap ran)
    HIPCHK(ctx, hipMemcpyAsync(uo, P->d_cand_count.p + gat::kCandSlots, gat::kStatUnitsOverlapWords * 8, hipMemcpyDeviceToHost, call_stream(ctx, P)));
  else std::fill(uo, uo + gat::kStatUnitsOverlapWords, 0ull);
  if (K.timed) HIPCHK(ctx, hipEventRecord(ctx->ev_cnt[1], call_stream(ctx, P)));
  K.main_rec[slot] = L.main_recorded; K.count_kernel[slot] = L.count_kernel;
  K.count_pending = false;
  if (K.enq == K.S) {
    // (the call's end rides on the last batch's synchronisation -- one round trip to the device less per call; a batch
    //  that has to be repeated enqueues it again)
    if (K.mstat_on) HIPCHK(ctx, hipMemcpyAsync(K.blk->h_mstat, P->d_mstat.p, 512 * 8, hipMemcpyDeviceToHost, call_stream(ctx, P)));
    HIPCHK(ctx, hipEventRecord(K.blk->ev_end, call_stream(ctx, P)));
    K.end_recorded = true;
  }
  return GAT_OK;
}

// Which count kernel will follow the next batch: it decides the sampler's last steps (final lists or not).  ONE rule, count_route,
// over what is known of the merged index: from the tables once they are built; while they are being built from what was announced
// of them -- will_merge alone where that says the merged index (many tracks, nucleotide counters: whatever the swap decision
// would be), with the announced sizes for the swap decision otherwise -- and with nothing announced the tables are waited for
static int next_batch_route(gat_ctx* ctx, gat_problem* P, const Counters& C, int* route) {
  gat_annotations* an = P->anno;
  const Knobs& kn = P->call.knobs;
  bool tables = annotations_ready(an);                       // decide from the tables themselves (built, or waited for)
  if (!tables) {
    if (count_route(ctx, kn, an->will_merge, C, P->n_contigs, P->n_tracks, 0) == GAT_COUNT_KERNEL_MERGED) { *route = GAT_COUNT_KERNEL_MERGED; return GAT_OK; }
    tables = !(an->shape_known && an->total_known >= 0);
  }
  if (tables) { const int rc = annotations_wait(ctx, an); if (rc) return rc; }
  decide_swap(P);                                            // (announced: from the sizes known before the build)
  *route = count_route(ctx, kn, tables ? an->dev.has_merged : an->will_merge, C, P->n_contigs, P->n_tracks, call_swap_capx(ctx, P),
                       tables && !an->dev.per_track);
  return GAT_OK;
}

// units_direct: the buffer of the candidates k_contig notes for k_units_overlap -- segments with a workspace boundary in their cells,
// of units that have a segment reaching out of their workspace: a fraction of a per cent of a batch's segments on isochore blocks
// much longer than the segments --, dealt to kCandSlots regions by (sample, contig).  Sized for THIS batch (a call's first batch is
// its largest; a later, larger call makes it anew while nothing of the problem is in flight); a region that overflows anyway has
// the batch repeated with four times the buffer (cand_scale), and beyond 64 times through the sorted contig lists
static int size_candidate_buffer(gat_ctx* ctx, gat_problem* P, int64_t nb) {
  double est = 0.006 * (double)nb * (double)std::max<int64_t>(1, P->n_seg_total) / gat::kCandSlots + 512.0;
  if (P->call.knobs.test_small_caps) est = 1.0;        // (tests: regions that overflow, the batch repeated with larger ones)
  const size_t want = (size_t)std::min(est * P->cand_scale, 1024.0 * 1024) * gat::kCandSlots;
  if (P->d_cand.n < want && P->call.n_flight == 0) {
    if (P->d_cand.n > 0) HIPCHK(ctx, hipStreamSynchronize(call_stream(ctx, P)));   // (an earlier call's kernels may still read the old buffer)
    HIPCHK(ctx, P->d_cand.alloc(want));
  }
  if (P->d_cand_count.n == 0) {
    HIPCHK(ctx, P->d_cand_count.alloc(gat::kCandSlots + 4));
    HIPCHK(ctx, hipMemsetAsync(P->d_cand_count.p, 0, (gat::kCandSlots + 4) * 4, call_stream(ctx, P)));
  }
  return GAT_OK;
}

// The sampler kernels of the next batch, their last steps by the count kernel that will follow (route), into the next free slot
static int enqueue_sampler_stage(gat_ctx* ctx, gat_problem* P, const Counters& C, int route) {
  CallState& K = P->call;
  const Knobs& kn = K.knobs;
  int rc;
  // the scratch is sized while nothing of this problem is in flight; batches behind the first fit by construction
  if (K.n_flight == 0 && (rc = ensure_scratch(ctx, P, kn, K.S - K.enq))) return rc;
  const int64_t nb = std::min<int64_t>(P->batch, K.S - K.enq);
  const int slot = K.n_flight;
  // (the run's one stream: the state at the batch's start is kept, a repeated batch draws from there)
  uint32_t* d_state = K.state_host != nullptr ? P->d_serial.p : nullptr;
  if (d_state != nullptr)
    HIPCHK(ctx, hipMemcpyAsync(d_state + GAT_MT_STATE_WORDS, d_state, GAT_MT_STATE_WORDS * 4, hipMemcpyDeviceToDevice, call_stream(ctx, P)));
  BatchOpts o;
  o.defer = true;                      // (enqueued only)
  // counts alone, all of them k_count_seg's: it reads the units as k_tail left them (no final lists are written)
  o.records_ok = !C.any_anno && !kn.count_final_lists && (route == GAT_COUNT_KERNEL_SEG || route == GAT_COUNT_KERNEL_MERGED);
  // (k_count_merged skips empty segments: long lists may keep what a trim emptied, no compaction pass in k_resume_big)
  o.loose_ok = o.records_ok && route == GAT_COUNT_KERNEL_MERGED;
  // isochore problems: the merged index takes the units' lists as they are, no k_contig (round 6)
  o.units_direct = o.loose_ok && P->merge_contigs && P->units_direct_ok && !kn.count_via_contigs;
  if (o.units_direct && (rc = size_candidate_buffer(ctx, P, nb))) return rc;
  o.serial_state = d_state;
  o.h_stat = K.blk->stat_slot(slot);
  if ((rc = run_sampler_batch(ctx, P, kn, K.seed, K.begin + K.enq, nb, &K.local, K.timed, o))) return rc;
  K.nb[slot] = nb;
  K.main_rec[slot] = false; K.count_kernel[slot] = GAT_COUNT_KERNEL_NONE;
  K.n_flight = slot + 1;
  K.enq += nb;
  K.count_pending = true;
  return GAT_OK;
}

// The scheduler: count kernels of the newest batch, sampler kernels of the next, until the call is enqueued or its flight is full.
// block: wait for annotation tables that are still being built (gat_wait); else return with the newest batch's count
// kernels still to come (gat_sample_and_count_enqueue: the host goes on, the device samples)
static int call_enqueue_more(gat_ctx* ctx, gat_problem* P, bool block) {
  CallState& K = P->call;
  Counters C;
  int rc = parse_counters(ctx, K.ids, K.n_counters, C);
  if (rc) return rc;
  // (the events behind every kernel and the serial stream's saved state exist once: such calls keep one batch in flight)
  const int max_flight = (K.timed || K.state_host != nullptr) ? 1 : kMaxInflight;
  PrepTimer tm;
  // (a layout made again was uploaded on the context's stream: it has arrived before a lane's kernels read it)
  if (K.lane >= 0) HIPCHK(ctx, stage_flush(ctx));
  for (;;) {
    if (K.count_pending) {
      if (!annotations_ready(P->anno) && !block) break;
      if ((rc = enqueue_count_stage(ctx, P, C))) return rc;
    }
    if (!(K.enq < K.S && K.n_flight < max_flight)) break;
    int route;
    if ((rc = next_batch_route(ctx, P, C, &route))) return rc;
    if ((rc = enqueue_sampler_stage(ctx, P, C, route))) return rc;
  }
  tm.lap("batches enqueued");
  return GAT_OK;
}

static void call_end(gat_ctx* ctx, gat_problem* P) {
  CallState& K = P->call;
  if (K.blk) ctx->call_blocks.push_back(K.blk);
  K.blk = nullptr;
  if (K.active) {
    ctx->calls_in_flight -= 1;
    if (K.lane >= 0) ctx->lane_calls[K.lane] -= 1;
  }
  K.lane = -1;
  K.active = false;
  if (ctx->timed_owner == (const void*)P) ctx->timed_owner = nullptr;
}

static int call_begin(gat_ctx* ctx, gat_problem* P, const int32_t* counter_ids, int n_counters, uint32_t seed,
                      int64_t sample_begin, int64_t sample_end, void* counts_dev, uint32_t* state_host, bool asynchronous) {
  if (!ctx || !P || !counts_dev || (n_counters > 0 && !counter_ids)) return set_err(ctx, GAT_ERR_ARG, "gat_sample_and_count: NULL argument");
  if (sample_end < sample_begin) return set_err(ctx, GAT_ERR_ARG, "sample_end < sample_begin");
  if (n_counters < 0 || n_counters > GAT_NUM_COUNTERS) return set_err(ctx, GAT_ERR_ARG, "%d counters (0..%d)", n_counters, GAT_NUM_COUNTERS);
  if (P->ctx != ctx) return set_err(ctx, GAT_ERR_ARG, "the problem was created on another context");
  CallState& K = P->call;
  if (K.active) return set_err(ctx, GAT_ERR_ARG, "a call is in flight on this problem: gat_wait first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Counters C;
  int rc = parse_counters(ctx, counter_ids, n_counters, C);
  if (rc) return rc;
  if (P->sampler == GAT_SAMPLER_SEGMENTS && !P->merge_contigs && n_counters > 0)
    return set_err(ctx, GAT_ERR_ASSERT, "SamplerSegments output is not normalized unless fromIsochores merges it "
                   "(keys without isochores): the counters assert (gat/SegmentList.pyx:1031)");
  if ((rc = call_block_get(ctx, &K.blk))) return rc;
  K.active = true;
  K.lane = -1;
  K.fork_waited = false;
  ctx->calls_in_flight += 1;                       // (this one included: call_end takes it off)
  K.knobs = read_knobs(ctx);                       // the call's: every batch of it, the ones gat_wait enqueues too
  for (int i = 0; i < n_counters; ++i) K.ids[i] = counter_ids[i];
  K.n_counters = n_counters;
  K.seed = seed; K.begin = sample_begin; K.S = sample_end - sample_begin;
  K.counts_dev = counts_dev; K.state_host = state_host;
  K.done = K.enq = 0; K.n_flight = 0;
  memset(&K.local, 0, sizeof(K.local));
  // (an event behind every kernel of the sampler costs 50-60 us of a call: 2 % at 10 000 samples of config 2, 6 % at 1 250)
  const bool times_wanted = ctx->kernel_times || K.knobs.kernel_times;
  K.timed = times_wanted && ctx->timed_owner == nullptr;
  if (K.timed) ctx->timed_owner = (const void*)P;
  // (the per-kernel events exist once per context: a call enqueued while another problem's timed call is in flight runs
  //  untimed -- its ms_* split reads 0 -- and says so: gat_stats::kernel_times)
  K.times_state = !times_wanted ? 0 : (K.timed ? 1 : -1);
  K.mstat_on = false;                              // (set with the first count kernels: it takes the tables)
  K.count_pending = false;
  K.end_recorded = false;
  // (a call that failed half enqueued: what it put on a lane has run before the problem's next call, on whatever stream, starts)
  auto fail = [&](int code) { if (K.lane >= 0) (void)hipStreamSynchronize(call_stream(ctx, P)); call_end(ctx, P); return code; };
  {
    bool busy[kMaxLanes];
    for (int l = 0; l < kMaxLanes; ++l) busy[l] = ctx->lane_calls[l] > 0;
    const int lane = K.S > 0 ? call_lane_for((int)K.knobs.call_lanes, asynchronous, times_wanted, state_host != nullptr, ctx->calls_in_flight - 1, busy) : -1;
    if (lane >= 0) {
      if (ctx->lanes[lane] == nullptr && hipStreamCreateWithFlags(&ctx->lanes[lane], hipStreamNonBlocking) != hipSuccess)
        return fail(set_err(ctx, GAT_ERR_DEVICE, "hipStreamCreateWithFlags failed (call lane %d)", lane));
      if (hipEventRecord(K.blk->ev_fork, ctx->stream) != hipSuccess) return fail(set_err(ctx, GAT_ERR_DEVICE, "hipEventRecord failed"));
      K.lane = lane;
      ctx->lane_calls[lane] += 1;
    }
  }
  if (hipEventRecord(K.blk->ev_begin, call_stream(ctx, P)) != hipSuccess) return fail(set_err(ctx, GAT_ERR_DEVICE, "hipEventRecord failed"));
  if (state_host != nullptr) {
    // the run's one stream: its state lives on the device over the batches (a copy restores it when a batch is repeated)
    if (P->d_serial.n < 2 * (size_t)GAT_MT_STATE_WORDS && P->d_serial.alloc(2 * (size_t)GAT_MT_STATE_WORDS) != hipSuccess)
      return fail(set_err(ctx, GAT_ERR_MEMORY, "device memory for the stream's state"));
    if (staged_h2d(ctx, P->d_serial.p, state_host, GAT_MT_STATE_WORDS * 4) != hipSuccess) return fail(set_err(ctx, GAT_ERR_DEVICE, "upload of the stream's state failed"));
  }
  if (K.S == 0) {                                                  // (no batch will run: nothing to ride on)
    if (hipEventRecord(K.blk->ev_end, ctx->stream) != hipSuccess) return fail(set_err(ctx, GAT_ERR_DEVICE, "hipEventRecord failed"));
    K.end_recorded = true;
    return GAT_OK;
  }
  if ((rc = call_enqueue_more(ctx, P, false))) return fail(rc);
  if (K.lane >= 0) {
    // the join: what the caller puts on its stream from here on is behind what this enqueue put on the lane (what gat_wait
    // enqueues later -- count kernels that waited for the tables, batches beyond kMaxInflight, repeats -- it also waits for)
    if (hipEventRecord(K.blk->ev_join, call_stream(ctx, P)) != hipSuccess || hipStreamWaitEvent(ctx->stream, K.blk->ev_join, 0) != hipSuccess)
      return fail(set_err(ctx, GAT_ERR_DEVICE, "joining the call's lane failed"));
  }
  return GAT_OK;
}

static int call_wait(gat_ctx* ctx, gat_problem* P, gat_stats* stats) {
  if (!ctx || !P) return set_err(ctx, GAT_ERR_ARG, "gat_wait: NULL argument");
  CallState& K = P->call;
  if (!K.active) return set_err(ctx, GAT_ERR_ARG, "gat_wait: no call in flight on this problem");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // (a failed call returns no counts; its statistics as far as they go are written: SamplerBruteForce's n_unconverged)
  auto fail = [&](int code) { (void)hipStreamSynchronize(call_stream(ctx, P)); if (stats) *stats = K.local; call_end(ctx, P); return code; };
  PrepTimer tm;
  int rc;
  if (K.count_pending && (rc = call_enqueue_more(ctx, P, true))) return fail(rc);   // (the tables were still being built)
  for (;;) {
    // ONE synchronisation per flight of batches: a sampler's status word is read behind the count kernels, which ran on
    // whatever an overflowed unit left.  What it left is in bounds: the exits that set a status bit (region full, a contig's
    // lists beyond the launch's LDS) leave unit_n / contig_n / the hand-over records as an EARLIER batch of this layout wrote
    // them -- lengths within the regions of this layout -- or as ensure_scratch zeroed them: a new layout (layout_slab +
    // upload_layout) sets P->batch = 0, so the scratch is sized and zeroed again before the next kernel runs, and no length
    // written under another layout survives into this one.  The counts of such a batch, and of the batches enqueued behind
    // it, are thrown away (they are redone)
    // (the call's own end where it is on the stream -- its last batch enqueued --, not the stream's: another problem's call
    //  enqueued behind this one -- run() keeps two segment tracks in flight, bench.py two steps -- goes on running while the
    //  host reads this one's status words and enqueues the next)
    const hipError_t se = K.end_recorded ? hipEventSynchronize(K.blk->ev_end) : hipStreamSynchronize(call_stream(ctx, P));
    if (se != hipSuccess) return fail(set_err(ctx, GAT_ERR_DEVICE, "synchronising with the call's batches failed: %s", hipGetErrorString(hipGetLastError())));
    K.end_recorded = false;
    tm.lap("batches synchronised");
    for (int slot = 0; slot < K.n_flight; ++slot) {
      rc = finish_sampler_batch(ctx, P, K.knobs, K.nb[slot], &K.local, K.timed, K.blk->stat_slot(slot));
      if (rc == kRelayout) {
        if (K.state_host != nullptr)        // (the repeated batch draws from where this one began)
          if (hipMemcpyAsync(P->d_serial.p, P->d_serial.p + GAT_MT_STATE_WORDS, GAT_MT_STATE_WORDS * 4, hipMemcpyDeviceToDevice, call_stream(ctx, P)) != hipSuccess)
            return fail(set_err(ctx, GAT_ERR_DEVICE, "restoring the stream's state failed"));
        break;
      }
      if (rc) return fail(rc);
      float ms = 0;
      if (K.timed && hipEventElapsedTime(&ms, ctx->ev_cnt[0], ctx->ev_cnt[1]) == hipSuccess) K.local.ms_count += ms;
      if (K.main_rec[slot] && hipEventElapsedTime(&ms, K.blk->ev_main[slot][0], K.blk->ev_main[slot][1]) == hipSuccess)
        K.local.ms_count_main += ms;
      K.local.count_kernel = K.count_kernel[slot];
      K.local.merged_form = K.count_kernel[slot] == GAT_COUNT_KERNEL_MERGED ? P->anno->dev.merged_block : 0;
      K.local.n_batches += 1;
      K.done += K.nb[slot];
    }
    K.n_flight = 0;
    K.enq = K.done;                                              // (what a repeated batch had behind it is enqueued again)
    if (K.done == K.S) break;
    if ((rc = call_enqueue_more(ctx, P, true))) return fail(rc);
  }
  if (K.state_host != nullptr && staged_d2h(ctx, K.state_host, P->d_serial.p, GAT_MT_STATE_WORDS * 4) != hipSuccess)
    return fail(set_err(ctx, GAT_ERR_DEVICE, "read-back of the stream's state failed"));
  if (K.mstat_on && K.S > 0)
    for (int i = 0; i < 256; ++i) { K.local.n_index_entries += (int64_t)K.blk->h_mstat[2 * i]; K.local.n_index_lookups += (int64_t)K.blk->h_mstat[2 * i + 1]; }
  float ms = 0;
  if (hipEventElapsedTime(&ms, K.blk->ev_begin, K.blk->ev_end) == hipSuccess) K.local.ms_total = ms; else (void)hipGetLastError();
  K.local.kernel_times = K.times_state;
  if (stats) *stats = K.local;
  call_end(ctx, P);
  return GAT_OK;
}

extern "C" int gat_sample_and_count_enqueue(gat_ctx* ctx, gat_problem* P, const int32_t* counter_ids, int n_counters,
                                            uint32_t seed, int64_t sample_begin, int64_t sample_end, void* counts_dev) {
  return call_begin(ctx, P, counter_ids, n_counters, seed, sample_begin, sample_end, counts_dev, nullptr, true);
}

extern "C" int gat_wait(gat_ctx* ctx, gat_problem* P, gat_stats* stats) { return call_wait(ctx, P, stats); }

extern "C" int gat_sample_and_count(gat_ctx* ctx, gat_problem* P, const int32_t* counter_ids, int n_counters,
                                    uint32_t seed, int64_t sample_begin, int64_t sample_end, void* counts_dev,
                                    gat_stats* stats) {
  const int rc = call_begin(ctx, P, counter_ids, n_counters, seed, sample_begin, sample_end, counts_dev, nullptr, false);
  return rc ? rc : call_wait(ctx, P, stats);
}

extern "C" int gat_sample_and_count_serial(gat_ctx* ctx, gat_problem* P, const int32_t* counter_ids, int n_counters,
                                           uint32_t* mt_state, int64_t n_samples, void* counts_dev, gat_stats* stats) {
  if (!mt_state) return set_err(ctx, GAT_ERR_ARG, "gat_sample_and_count_serial: NULL state");
  if (sampler_runs_wave_per_unit(P->sampler))                 // (the list samplers: no k_serial)
    return set_err(ctx, GAT_ERR_ARG, "gat_sample_and_count_serial: %s runs on the per-unit streams only", sampler_info(P->sampler)->name);
  if (mt_state[GAT_MT_STATE_WORDS - 1] > 624u) return set_err(ctx, GAT_ERR_ARG, "gat_sample_and_count_serial: position %u > 624", mt_state[GAT_MT_STATE_WORDS - 1]);
  const int rc = call_begin(ctx, P, counter_ids, n_counters, 0u, 0, n_samples, counts_dev, mt_state, false);
  return rc ? rc : call_wait(ctx, P, stats);
}

extern "C" void gat_mt19937_seed(uint32_t seed, uint32_t* mt_state) {
  // numpy.random.seed(int): init_genrand (numpy/random/src/mt19937/mt19937.c: mt19937_seed), position = 624
  uint32_t x = seed;
  for (int i = 0; i < 624; ++i) { mt_state[i] = x; x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)(i + 1); }
  mt_state[624] = 624u;
}

#include "gat_list_calls.h"   // gat_sample and the list reductions: gat_sample_* / gat_list_*

// what gat_count_lists / gat_count_list_ranges were given, as it goes down to the launches
struct CountListsIn {
  const int32_t* counter_ids; int n_counters;
  const gat_segment* lists; const int64_t* list_off; int64_t n_lists;
  const gat_segment* annos; const int64_t *anno_begin, *anno_end; int32_t n_tracks;
  const int64_t* ws_nseg; int32_t n_groups;
  void* counts_host;
};
// The device buffers of a gat_count_lists call.  They go back to the process-wide pool when they are destroyed, and the pool
// hands an idle block to any context or stream: on EVERY path out of the call -- an error in the middle of its launches
// too -- the stream is drained before that (count_lists_on owns them and synchronises behind count_lists_body: ADVICE r4)
struct CountListBufs {
  AnnoDev A;
  DevBuf<uint2> d_seg;
  DevBuf<int32_t> d_c_off, d_n, d_index;
  DevBuf<int64_t> d_nseg, d_out;
  DevBuf<uint32_t> d_part;
};
static int count_lists_body(gat_ctx* ctx, const Knobs& kn, const CountListsIn& in, CountListBufs& B) {
  const int64_t n_lists = in.n_lists;
  const int32_t n_groups = in.n_groups, n_tracks = in.n_tracks;
  Counters C;
  int rc = parse_counters(ctx, in.counter_ids, in.n_counters, C);
  if (rc) return rc;
  // (the merged index pays when many lists are counted against it; for a handful -- the observed counts of a run's
  //  segment tracks -- building it costs more than the per-track kernel's extra look-ups)
  const bool want_merged = n_lists >= 16 || kn.count_lists_merged;
  if ((rc = build_annos(ctx, kn, B.A, in.annos, in.anno_begin, in.anno_end, (int64_t)n_tracks * n_groups, n_groups, want_merged, false))) return rc;
  for (int64_t l = 0; l < n_lists * n_groups; ++l)
    if ((rc = check_list(ctx, in.lists + in.list_off[l], in.list_off[l + 1] - in.list_off[l], "segment", l))) return rc;
  const int64_t total = in.list_off[n_lists * n_groups];
  // (+1: k_count_seg issues the load of a list's element 0 whatever its length and turns it into padding afterwards -- an
  //  empty list behind the last segment read 8 bytes beyond the buffer)
  std::vector<uint2> h_seg((size_t)total + 1, make_uint2(0u, 0u));
  for (int64_t i = 0; i < total; ++i) h_seg[(size_t)i] = make_uint2(in.lists[i].start, in.lists[i].end);
  HIPCHK(ctx, B.d_seg.upload(h_seg, ctx));
  std::vector<int64_t> h_nseg(in.ws_nseg, in.ws_nseg + n_groups);
  HIPCHK(ctx, B.d_nseg.upload(h_nseg, ctx));
  const size_t nslots = (size_t)in.n_counters * n_tracks * n_lists;
  HIPCHK(ctx, B.d_out.alloc(nslots));
  HIPCHK(ctx, hipMemsetAsync(B.d_out.p, 0, std::max<size_t>(1, nslots) * 8, ctx->stream));
  std::vector<int32_t> h_index((size_t)n_groups);
  for (int g = 0; g < n_groups; ++g) h_index[(size_t)g] = g;
  HIPCHK(ctx, B.d_index.upload(h_index, ctx));
  // the group offsets and lengths of every list, uploaded once; one launch per list (they differ from list to list)
  std::vector<int32_t> h_c_off((size_t)std::max<int64_t>(1, n_lists * n_groups)), h_n((size_t)std::max<int64_t>(1, n_lists * n_groups));
  for (int64_t l = 0; l < n_lists; ++l) {
    const int64_t base = in.list_off[l * n_groups];
    for (int g = 0; g < n_groups; ++g) {
      h_c_off[(size_t)(l * n_groups + g)] = (int32_t)(in.list_off[l * n_groups + g] - base);
      h_n[(size_t)(l * n_groups + g)] = (int32_t)(in.list_off[l * n_groups + g + 1] - in.list_off[l * n_groups + g]);
    }
  }
  HIPCHK(ctx, B.d_c_off.upload(h_c_off, ctx));
  HIPCHK(ctx, B.d_n.upload(h_n, ctx));
  for (int64_t l = 0; l < n_lists; ++l) {
    const int64_t base = in.list_off[l * n_groups];
    gat::CountArgs K;
    memset(&K, 0, sizeof(K));
    K.seg = B.d_seg.p + base; K.seg_stride = 0; K.c_off = B.d_c_off.p + l * n_groups;
    K.n_arr = B.d_n.p + l * n_groups; K.n_stride = 0; K.n_index = B.d_index.p;
    K.cws_nseg = B.d_nseg.p; K.n_contigs = n_groups; K.n_tracks = n_tracks; K.n_samples = 1;
    K.out = B.d_out.p; K.out_stride = n_lists; K.out_begin = l;
    int32_t longest = 0;
    for (int g = 0; g < n_groups; ++g) longest = std::max(longest, h_n[(size_t)(l * n_groups + g)]);
    CountLaunch L;
    L.stream = ctx->stream;
    L.ev_main = ctx->ev_main;
    if ((rc = launch_count(ctx, kn, B.A, C, K, B.d_part, 0, longest, L))) return rc;
  }
  HIPCHK(ctx, staged_d2h(ctx, in.counts_host, B.d_out.p, nslots * 8));
  return GAT_OK;
}

static int count_lists_on(gat_ctx* ctx, const Knobs& kn, const CountListsIn& in) {
  CountListBufs B;
  const int rc = count_lists_body(ctx, kn, in, B);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// Observed counts are independent of whatever samples are in flight on the caller's context: they run on a stream (and
// through a staging buffer) of their own -- every staged upload waits for its stream, and on the caller's stream that would
// be the end of the sampling (run() computes them while the device samples, gat/__init__.py:933-940)
static int count_lists_impl(gat_ctx* ctx, const CountListsIn& in) {
  if (!ctx || !in.list_off || !in.anno_begin || !in.anno_end || !in.counts_host || (in.n_groups > 0 && !in.ws_nseg))
    return set_err(ctx, GAT_ERR_ARG, "gat_count_lists: NULL argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->aux_ctx == nullptr) {
    int rc = gat_ctx_create(&ctx->aux_ctx, ctx->device, nullptr);
    if (rc) return rc;
  }
  gat_ctx* x = ctx->aux_ctx;
  const Knobs kn = read_knobs(ctx);                 // (the caller's: the auxiliary context has no options of its own)
  x->count_report = gat_count_report();             // (a call without a list launches nothing)
  const int rc = count_lists_on(x, kn, in);
  ctx->count_report = x->count_report;
  x->stage_used = 0;                                // (count_lists_on has drained the stream before its buffers went back to the pool)
  if (rc) return set_err(ctx, rc, "%s", x->err.c_str());
  return GAT_OK;
}

extern "C" int gat_count_lists(gat_ctx* ctx, const int32_t* counter_ids, int n_counters,
                               const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                               const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                               const int64_t* ws_nseg, int32_t n_groups, void* counts_host) {
  if (!anno_off) return set_err(ctx, GAT_ERR_ARG, "gat_count_lists: NULL argument");
  return count_lists_impl(ctx, {counter_ids, n_counters, lists, list_off, n_lists, annos, anno_off, anno_off + 1, n_tracks, ws_nseg, n_groups, counts_host});
}

extern "C" int gat_count_last_launch(const gat_ctx* ctx, gat_count_report* out) {
  if (!ctx || !out) return set_err(nullptr, GAT_ERR_ARG, "gat_count_last_launch: NULL argument");
  *out = ctx->count_report;
  return GAT_OK;
}

extern "C" int gat_sampler_last_launch(const gat_ctx* ctx, gat_sampler_report* out) {
  if (!ctx || !out) return set_err(nullptr, GAT_ERR_ARG, "gat_sampler_last_launch: NULL argument");
  *out = ctx->sampler_report;
  return GAT_OK;
}

extern "C" int gat_count_list_ranges(gat_ctx* ctx, const int32_t* counter_ids, int n_counters,
                                     const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                     const gat_segment* annos, const int64_t* anno_begin, const int64_t* anno_end, int32_t n_tracks,
                                     const int64_t* ws_nseg, int32_t n_groups, void* counts_host) {
  return count_lists_impl(ctx, {counter_ids, n_counters, lists, list_off, n_lists, annos, anno_begin, anno_end, n_tracks, ws_nseg, n_groups, counts_host});
}

// ------------------------------------------------------------------------------------------
// The one collective of the path: all-gather of the per-rank count blocks over xGMI (RCCL), replacing the reference's
// pool result collation (gat/__init__.py:681-700, :770-774).  RCCL is loaded lazily so that single-GPU hosts need not
// have it (and so that a process that already holds torch's copy does not get a second one by linking).
struct RcclApi {
  void* handle = nullptr;
  bool preloaded = false;      // the library was in the process already (torch's copy, or one the host linked)
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};
static RcclApi* rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (!tried) {
    tried = true;
    // A process must not hold two RCCLs (two sets of communicators' bootstrap state, two IPC caches): where one is mapped
    // already -- torch brings its own copy, torch/lib/librccl.so, and resolves it by that name -- that one is taken:
    // RTLD_NOLOAD returns a handle only for a library that is loaded, by soname or by the path it was loaded from.  Failing
    // that, any object of the process that exports the entry points (RTLD_DEFAULT: a host that linked RCCL itself); only then
    // is a library loaded afresh.  GAT_RCCL_LIB names one explicitly.
    const std::string& env_lib = process_knobs().rccl_lib;
    if (!env_lib.empty()) api.handle = dlopen(env_lib.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!api.handle)
      for (const char* name : {"librccl.so", "librccl.so.1"}) {
        api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (api.handle) break;
      }
    if (!api.handle) {
      // (mapped under a path dlopen does not search -- torch/lib --: find it among the process's objects)
      struct Find { std::string path; } f;
      dl_iterate_phdr([](struct dl_phdr_info* info, size_t, void* data) -> int {
        const char* nm = info->dlpi_name;
        if (nm && strstr(nm, "librccl.so")) { static_cast<Find*>(data)->path = nm; return 1; }
        return 0;
      }, &f);
      if (!f.path.empty()) api.handle = dlopen(f.path.c_str(), RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    }
    api.preloaded = api.handle != nullptr;
    if (!api.handle && dlsym(RTLD_DEFAULT, "ncclAllGather") != nullptr) { api.handle = RTLD_DEFAULT; api.preloaded = true; }
    if (!api.handle)
      for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (api.handle) break;
      }
    if (api.handle || api.preloaded) {
      api.get_unique_id = (decltype(api.get_unique_id))dlsym(api.handle, "ncclGetUniqueId");
      api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(api.handle, "ncclCommInitRank");
      api.comm_destroy = (decltype(api.comm_destroy))dlsym(api.handle, "ncclCommDestroy");
      api.all_gather = (decltype(api.all_gather))dlsym(api.handle, "ncclAllGather");
      api.error_string = (decltype(api.error_string))dlsym(api.handle, "ncclGetErrorString");
    }
  }
  const bool ok = (api.handle || api.preloaded) && api.get_unique_id && api.comm_init_rank && api.comm_destroy && api.all_gather;
  return ok ? &api : nullptr;
}

// which RCCL gat_comm_* resolved: 1 one the process had mapped already (RTLD_NOLOAD / among its objects), 0 loaded afresh, -1 none
extern "C" int gat_comm_library_preloaded(void) {
  RcclApi* R = rccl_api();
  return R ? (R->preloaded ? 1 : 0) : -1;
}

struct gat_comm {
  ncclComm_t comm = nullptr;
  int n_ranks = 1, rank = 0;
};

static_assert(sizeof(ncclUniqueId) == GAT_COMM_ID_BYTES, "GAT_COMM_ID_BYTES");

extern "C" int gat_comm_unique_id(void* id_out) {
  if (!id_out) return set_err(nullptr, GAT_ERR_ARG, "gat_comm_unique_id: NULL argument");
  RcclApi* R = rccl_api();
  if (!R) return set_err(nullptr, GAT_ERR_DEVICE, "RCCL (librccl.so) is not available: %s", dlerror() ? dlerror() : "symbols missing");
  ncclUniqueId id;
  const ncclResult_t rc = R->get_unique_id(&id);
  if (rc != ncclSuccess) return set_err(nullptr, GAT_ERR_DEVICE, "ncclGetUniqueId: %s", R->error_string ? R->error_string(rc) : "error");
  memcpy(id_out, &id, sizeof(id));
  return GAT_OK;
}

extern "C" int gat_comm_create(gat_ctx* ctx, gat_comm** out, int n_ranks, int rank, const void* id) {
  if (!ctx || !out || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return set_err(ctx, GAT_ERR_ARG, "gat_comm_create: bad argument");
  *out = nullptr;
  RcclApi* R = rccl_api();
  if (!R) return set_err(ctx, GAT_ERR_DEVICE, "RCCL (librccl.so) is not available");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  std::unique_ptr<gat_comm> C(new gat_comm());
  C->n_ranks = n_ranks;
  C->rank = rank;
  const ncclResult_t rc = R->comm_init_rank(&C->comm, n_ranks, uid, rank);
  if (rc != ncclSuccess) return set_err(ctx, GAT_ERR_DEVICE, "ncclCommInitRank: %s", R->error_string ? R->error_string(rc) : "error");
  *out = C.release();
  return GAT_OK;
}

extern "C" void gat_comm_destroy(gat_comm* comm) {
  if (!comm) return;
  RcclApi* R = rccl_api();
  if (R && comm->comm) (void)R->comm_destroy(comm->comm);
  delete comm;
}

extern "C" int gat_allgather_counts(gat_ctx* ctx, gat_comm* comm, const void* send_dev, void* recv_dev, int64_t n_slots) {
  if (!ctx || !comm || !send_dev || !recv_dev || n_slots < 0) return set_err(ctx, GAT_ERR_ARG, "gat_allgather_counts: bad argument");
  RcclApi* R = rccl_api();
  if (!R) return set_err(ctx, GAT_ERR_DEVICE, "RCCL (librccl.so) is not available");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const ncclResult_t rc = R->all_gather(send_dev, recv_dev, (size_t)n_slots, ncclInt64, comm->comm, ctx->stream);
  if (rc != ncclSuccess) return set_err(ctx, GAT_ERR_DEVICE, "ncclAllGather: %s", R->error_string ? R->error_string(rc) : "error");
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return GAT_OK;
}

// ------------------------------------------------------------------------------------------
// numpy's pairwise summation of a block of `n` elements starting at `off` (numpy/_core/src/umath/loops_utils.h.src,
// pairwise_sum): the blocks of at most 128 elements and the order in which their sums are added
static void np_pairwise_plan(int off, int n, std::vector<int32_t>& leaf_off, std::vector<int32_t>& leaf_len, std::vector<int32_t>& prog) {
  if (n <= gat::kNpBlock) {
    prog.push_back((int32_t)leaf_off.size());
    leaf_off.push_back(off);
    leaf_len.push_back(n);
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  np_pairwise_plan(off, n2, leaf_off, leaf_len, prog);
  np_pairwise_plan(off + n2, n - n2, leaf_off, leaf_len, prog);
  prog.push_back(-1);
}

// what a launch of k_null_stats over rows of n_samples needs beside the rows: the plan of the last, partial chunk on the
// device, the dynamic LDS, the kernel's attribute set.  `who`: the entry's name for the message
struct StatsPlan {
  DevBuf<int32_t> d_off, d_len, d_prog;
  int32_t n_leaves = 0, n_prog = 0;
  size_t lds = 0;
  void fill(gat::StatsArgs& A) const { A.leaf_off = d_off.p; A.leaf_len = d_len.p; A.n_leaves = n_leaves; A.prog = d_prog.p; A.n_prog = n_prog; }
};
static int stats_plan(gat_ctx* ctx, int64_t n_samples, StatsPlan& P, const char* who) {
  std::vector<int32_t> leaf_off, leaf_len, prog;
  const int rest = (int)(n_samples % gat::kNpChunk);
  if (rest > 0) np_pairwise_plan(0, rest, leaf_off, leaf_len, prog);
  if (leaf_off.empty()) { leaf_off.push_back(0); leaf_len.push_back(0); prog.push_back(0); }
  HIPCHK(ctx, P.d_off.upload(leaf_off, ctx));
  HIPCHK(ctx, P.d_len.upload(leaf_len, ctx));
  HIPCHK(ctx, P.d_prog.upload(prog, ctx));
  P.n_leaves = rest > 0 ? (int32_t)leaf_off.size() : 0;
  P.n_prog = rest > 0 ? (int32_t)prog.size() : 0;
  P.lds = (size_t)(n_samples / gat::kNpChunk + 1 + leaf_off.size()) * 8;
  if ((int64_t)P.lds > ctx->max_lds - 4096) return set_err(ctx, GAT_ERR_CAPACITY, "%s: %lld samples per row", who, (long long)n_samples);
  HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_null_stats, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
  return GAT_OK;
}

extern "C" int gat_null_stats(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples,
                              const uint8_t* is_double_host, const double* vals_host, int64_t lo_index, int64_t hi_index,
                              double* out_host) {
  if (!ctx || !counts_dev || !is_double_host || !vals_host || !out_host) return set_err(ctx, GAT_ERR_ARG, "gat_null_stats: NULL argument");
  if (n_rows <= 0) return GAT_OK;
  if (n_samples < 1 || n_samples >= ((int64_t)1 << 31) || lo_index < 0 || hi_index < 0 || lo_index >= n_samples || hi_index >= n_samples)
    return set_err(ctx, GAT_ERR_ARG, "gat_null_stats: bad sample count / positions");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  StatsPlan plan;
  DevBuf<uint8_t> d_dbl;
  DevBuf<double> d_vals, d_out;
  { const int rc = stats_plan(ctx, n_samples, plan, "gat_null_stats"); if (rc != GAT_OK) return rc; }
  HIPCHK(ctx, d_dbl.upload(std::vector<uint8_t>(is_double_host, is_double_host + n_rows), ctx));
  HIPCHK(ctx, d_vals.upload(std::vector<double>(vals_host, vals_host + n_rows), ctx));
  HIPCHK(ctx, d_out.alloc((size_t)n_rows * 8));
  gat::StatsArgs A;
  A.counts = (const int64_t*)counts_dev; A.row_stride = n_samples; A.n_rows = (int32_t)n_rows; A.S = (int32_t)n_samples;
  A.is_double = d_dbl.p; A.vals = d_vals.p; A.out = d_out.p; A.lo_i = (int32_t)lo_index; A.hi_i = (int32_t)hi_index;
  plan.fill(A);
  for (int64_t r0 = 0; r0 < n_rows; r0 += 1 << 20) {               // (grid x: rows)
    gat::StatsArgs B = A;
    const int64_t nr = std::min<int64_t>(n_rows - r0, 1 << 20);
    B.counts = A.counts + r0 * n_samples; B.is_double = A.is_double + r0; B.vals = A.vals + r0; B.out = A.out + r0 * 8; B.n_rows = (int32_t)nr;
    hipLaunchKernelGGL(gat::k_null_stats, dim3((unsigned)nr), dim3(gat::kStatsThreads), plan.lds, ctx->stream, B);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, staged_d2h(ctx, out_host, d_out.p, (size_t)n_rows * 64));
  return GAT_OK;
}

// A round of a count matrix folded into the rows' eight integer words (include/gat_mi355.h, gat_null_fold.h).
static_assert(gat::kNullFoldWords == GAT_NULL_FOLD_WORDS, "gat_null_fold.h and gat_mi355.h disagree on the words of a row");
extern "C" int gat_null_fold_reset(gat_ctx* ctx, uint64_t* words_dev, int64_t n_rows) {
  if (!ctx || !words_dev || n_rows < 0) return set_err(ctx, GAT_ERR_ARG, "gat_null_fold_reset: bad argument");
  if (n_rows == 0) return GAT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t n_words = n_rows * gat::kNullFoldWords;
  hipLaunchKernelGGL(gat::k_null_fold_reset, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, ctx->stream,
                     (unsigned long long*)words_dev, n_words);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return GAT_OK;
}

extern "C" int gat_null_fold(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples, int64_t row_stride,
                             const double* vals_host, uint64_t* words_dev) {
  if (!ctx || !counts_dev || !vals_host || !words_dev) return set_err(ctx, GAT_ERR_ARG, "gat_null_fold: NULL argument");
  if (n_rows < 0 || n_samples < 1 || row_stride < n_samples)
    return set_err(ctx, GAT_ERR_ARG, "gat_null_fold: bad row count / sample count / row stride");
  if (n_rows == 0) return GAT_OK;
  // val as two integers: v < val is v < lt, v == val is v == eq (gat_null_fold.h)
  std::vector<unsigned long long> lt((size_t)n_rows), eq((size_t)n_rows);
  for (int64_t r = 0; r < n_rows; ++r) {
    const double val = vals_host[r];
    if (!std::isfinite(val)) return set_err(ctx, GAT_ERR_ARG, "gat_null_fold: the value of row %lld is not finite", (long long)r);
    const double c = std::ceil(val);
    lt[(size_t)r] = c <= 0.0 ? 0ull : c >= 9223372036854775808.0 ? 1ull << 63 : (unsigned long long)c;
    eq[(size_t)r] = (c == val && c >= 0.0 && c < 9223372036854775808.0) ? (unsigned long long)c : gat::kNullFoldNoEq;
  }
  const Knobs kn = read_knobs(ctx);                 // the call's
  if (kn.null_fold_parts < 0 || kn.null_fold_parts > 1024) return set_err(ctx, GAT_ERR_ARG, "gat_null_fold: GAT_NULL_FOLD_PARTS must be 0 .. 1024");
  // a row is cut over several workgroups when the rows alone do not fill the device, down to 4 096 samples a workgroup
  int64_t parts = kn.null_fold_parts;
  if (parts == 0) parts = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(1024, 2048 / n_rows), n_samples / 4096));
  const int64_t chunk = (n_samples + parts - 1) / parts;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf<unsigned long long> d_lt, d_eq;
  HIPCHK(ctx, d_lt.upload(lt, ctx));
  HIPCHK(ctx, d_eq.upload(eq, ctx));
  gat::NullFoldArgs A;
  A.row_stride = row_stride; A.S = n_samples; A.chunk = chunk;
  for (int64_t r0 = 0; r0 < n_rows; r0 += 1 << 20) {                // (grid x: rows)
    const int64_t nr = std::min<int64_t>(n_rows - r0, 1 << 20);
    A.counts = (const unsigned long long*)counts_dev + r0 * row_stride; A.lt = d_lt.p + r0; A.eq = d_eq.p + r0;
    A.words = (unsigned long long*)words_dev + r0 * gat::kNullFoldWords;
    hipLaunchKernelGGL(gat::k_null_fold, dim3((unsigned)nr, (unsigned)parts), dim3(gat::kNullFoldThreads), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, stage_flush(ctx));                    // (the two uploads have left the staging buffer)
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return GAT_OK;
}

// gat-compare's statistics (include/gat_mi355.h): k_compare_rows fills a scratch block with the rows of a batch of pairs,
// k_null_stats reads it; the rows never leave the device.  The batch is what the call's GAT_COMPARE_SCRATCH_MB holds.
extern "C" int gat_compare_stats(gat_ctx* ctx, const void* a_dev, int64_t n_rows_a, const void* b_dev, int64_t n_rows_b,
                                 int64_t n_samples, const int32_t* ia_host, const int32_t* ib_host, int64_t n_pairs,
                                 const double* obs_a_host, const double* obs_b_host, const double* delta_host,
                                 double pseudo_count, int64_t lo_index, int64_t hi_index, double* out_host) {
  if (!ctx || !a_dev || !b_dev || !ia_host || !ib_host || !obs_a_host || !obs_b_host || !delta_host || !out_host)
    return set_err(ctx, GAT_ERR_ARG, "gat_compare_stats: NULL argument");
  if (n_pairs <= 0) return GAT_OK;
  if (n_samples < 1 || n_samples >= ((int64_t)1 << 31) - 1 || lo_index < 0 || hi_index < 0 || lo_index >= n_samples || hi_index >= n_samples)
    return set_err(ctx, GAT_ERR_ARG, "gat_compare_stats: bad sample count / positions");
  if (n_rows_a < 1 || n_rows_b < 1 || n_rows_a >= ((int64_t)1 << 31) || n_rows_b >= ((int64_t)1 << 31))
    return set_err(ctx, GAT_ERR_ARG, "gat_compare_stats: bad row counts");
  for (int64_t p = 0; p < n_pairs; ++p)
    if (ia_host[p] < 0 || ia_host[p] >= n_rows_a || ib_host[p] < 0 || ib_host[p] >= n_rows_b)
      return set_err(ctx, GAT_ERR_ARG, "gat_compare_stats: pair %lld names row (%d, %d) of (%lld, %lld)", (long long)p, ia_host[p],
                     ib_host[p], (long long)n_rows_a, (long long)n_rows_b);
  const Knobs kn = read_knobs(ctx);                 // the call's
  if (!(kn.compare_scratch_mb > 0.0)) return set_err(ctx, GAT_ERR_ARG, "gat_compare_stats: GAT_COMPARE_SCRATCH_MB must be positive");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t stride = (n_samples + 1) & ~(int64_t)1;             // even: every scratch row starts on a 16-byte boundary
  const double budget_rows = kn.compare_scratch_mb * 1048576.0 / (double)(stride * 8);
  const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_pairs, 1 << 20), budget_rows >= 1048576.0 ? (1 << 20) : (int64_t)budget_rows));
  StatsPlan plan;
  { const int rc = stats_plan(ctx, n_samples, plan, "gat_compare_stats"); if (rc != GAT_OK) return rc; }
  DevBuf<int32_t> d_ia, d_ib;
  DevBuf<double> d_oa, d_ob, d_delta, d_rows, d_out;
  DevBuf<uint8_t> d_dbl;
  DevBuf<uint32_t> d_bad;
  HIPCHK(ctx, d_ia.upload(std::vector<int32_t>(ia_host, ia_host + n_pairs), ctx));
  HIPCHK(ctx, d_ib.upload(std::vector<int32_t>(ib_host, ib_host + n_pairs), ctx));
  HIPCHK(ctx, d_oa.upload(std::vector<double>(obs_a_host, obs_a_host + n_pairs), ctx));
  HIPCHK(ctx, d_ob.upload(std::vector<double>(obs_b_host, obs_b_host + n_pairs), ctx));
  HIPCHK(ctx, d_delta.upload(std::vector<double>(delta_host, delta_host + n_pairs), ctx));
  HIPCHK(ctx, d_dbl.upload(std::vector<uint8_t>((size_t)batch, (uint8_t)1), ctx));
  HIPCHK(ctx, d_rows.alloc((size_t)batch * (size_t)stride));
  HIPCHK(ctx, d_out.alloc((size_t)n_pairs * 8));
  HIPCHK(ctx, d_bad.alloc((size_t)n_pairs));
  gat::CompareArgs C;
  C.a = (const double*)a_dev; C.b = (const double*)b_dev; C.S = (int32_t)n_samples; C.pseudo_count = pseudo_count;
  C.rows = d_rows.p; C.row_stride = stride;
  gat::StatsArgs A;
  A.counts = (const int64_t*)d_rows.p; A.row_stride = stride; A.S = (int32_t)n_samples; A.is_double = d_dbl.p;
  A.lo_i = (int32_t)lo_index; A.hi_i = (int32_t)hi_index;
  plan.fill(A);
  for (int64_t p0 = 0; p0 < n_pairs; p0 += batch) {                 // (one stream: a batch's rows are read before the next one's are written)
    const int64_t np = std::min<int64_t>(batch, n_pairs - p0);
    C.n_pairs = (int32_t)np; C.ia = d_ia.p + p0; C.ib = d_ib.p + p0; C.obs_a = d_oa.p + p0; C.obs_b = d_ob.p + p0; C.delta = d_delta.p + p0;
    C.n_nonfinite = d_bad.p + p0;
    hipLaunchKernelGGL(gat::k_compare_rows, dim3((unsigned)np), dim3(gat::kCompareThreads), 0, ctx->stream, C);
    HIPCHK(ctx, hipGetLastError());
    A.n_rows = (int32_t)np; A.vals = d_delta.p + p0; A.out = d_out.p + p0 * 8;
    hipLaunchKernelGGL(gat::k_null_stats, dim3((unsigned)np), dim3(gat::kStatsThreads), plan.lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, staged_d2h(ctx, out_host, d_out.p, (size_t)n_pairs * 64));
  std::vector<uint32_t> bad((size_t)n_pairs);
  HIPCHK(ctx, staged_d2h(ctx, bad.data(), d_bad.p, (size_t)n_pairs * 4));
  for (int64_t p = 0; p < n_pairs; ++p) out_host[p * 8 + 6] = (double)bad[(size_t)p];
  return GAT_OK;
}

// Step-down minP (include/gat_mi355.h, gat_minp.h): the rows are ordered on the host by (k_obs, row index) and worked on from
// the last of that order to the first, in batches of as many rows of K as the call's GAT_MINP_SCRATCH_MB holds; k_minp_rank
// fills the batch's rows of K, k_minp_step takes the running minimum q through them and counts.  q stays on the device from
// batch to batch; what comes back is one integer per row.
struct MinpTimer {                                  // device times of the two kernels, only for a call that asks (kernel times)
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~MinpTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  // ev[0] .. ev[1] around the first kernel, ev[1] .. ev[2] around the second: waits for the batch and adds to ms[0], ms[1]
  int add(gat_ctx* ctx, float* ms) {
    HIPCHK(ctx, hipEventRecord(ev[2], ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&a, ev[0], ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&b, ev[1], ev[2]));
    ms[0] += a; ms[1] += b;
    return GAT_OK;
  }
};

// "rank one batch of rows into K", the step gat_minp_counts and gat_efdr_counts share: the checks of the arguments and of the
// options both have (`who` names the entry in the error texts), the batch size, K and the sort scratch, and the launch of
// k_minp_rank for the batch rows a device array names.
struct MinpRanker {
  int64_t S = 0, batch = 0, grid_rank = 0;
  bool in_lds = false;
  size_t lds = 0;
  DevBuf<int32_t> d_K;
  DevBuf<uint8_t> d_dbl;
  DevBuf<double> d_means;
  DevBuf<unsigned long long> d_sort;
  gat::MinpRankArgs R;

  static int check(gat_ctx* ctx, const Knobs& kn, const char* who, int64_t n_rows, int64_t n_samples, const int32_t* kobs_host) {
    if (n_samples < 1 || n_samples >= ((int64_t)1 << 31) || n_rows >= ((int64_t)1 << 31))
      return set_err(ctx, GAT_ERR_ARG, "%s: bad sample / row count", who);
    for (int64_t r = 0; r < n_rows; ++r)
      if (kobs_host[r] < 1 || (int64_t)kobs_host[r] > n_samples)
        return set_err(ctx, GAT_ERR_ARG, "%s: row %lld has k_obs %d of %lld samples", who, (long long)r, kobs_host[r], (long long)n_samples);
    if (!(kn.minp_scratch_mb > 0.0)) return set_err(ctx, GAT_ERR_ARG, "%s: GAT_MINP_SCRATCH_MB must be positive", who);
    const int64_t lds_max = ((int64_t)ctx->max_lds - gat::kMinpLdsFixed) / gat::kMinpKeyBytes;
    if (kn.minp_lds_samples < 0 || kn.minp_lds_samples > lds_max)
      return set_err(ctx, GAT_ERR_ARG, "%s: GAT_MINP_LDS_SAMPLES must be in [0, %lld]", who, (long long)lds_max);
    return GAT_OK;
  }
  int init(gat_ctx* ctx, const Knobs& kn, const void* counts_dev, int64_t n_rows, int64_t n_samples,
           const uint8_t* is_double_host, const double* means_host) {
    S = n_samples;
    const double budget_rows = kn.minp_scratch_mb * 1048576.0 / (double)(S * 4);
    batch = std::max<int64_t>(1, budget_rows >= (double)n_rows ? n_rows : (int64_t)budget_rows);
    in_lds = S <= kn.minp_lds_samples;
    grid_rank = std::min<int64_t>(batch, gat::kMinpRankGrid);
    lds = (size_t)gat::kMinpLdsFixed + (in_lds ? (size_t)S * gat::kMinpKeyBytes : 0);
    HIPCHK(ctx, d_dbl.upload(std::vector<uint8_t>(is_double_host, is_double_host + n_rows), ctx));
    HIPCHK(ctx, d_means.upload(std::vector<double>(means_host, means_host + n_rows), ctx));
    HIPCHK(ctx, d_K.alloc((size_t)batch * (size_t)S));
    if (!in_lds) HIPCHK(ctx, d_sort.alloc((size_t)grid_rank * 2 * (size_t)S));
    if (in_lds) HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_minp_rank<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    R.counts = (const int64_t*)counts_dev; R.row_stride = S; R.S = (int32_t)S; R.is_double = d_dbl.p; R.means = d_means.p;
    R.K = d_K.p; R.sort_scratch = d_sort.p; R.skip_passes = kn.minp_all_passes ? 0 : 1;
    return GAT_OK;
  }
  // K[b] = the ranks of matrix row rows_dev[b], b < nb <= batch
  int launch(gat_ctx* ctx, const int32_t* rows_dev, int64_t nb) {
    R.n_rows = (int32_t)nb; R.rows = rows_dev;
    if (in_lds) hipLaunchKernelGGL(gat::k_minp_rank<true>, dim3((unsigned)std::min<int64_t>(nb, grid_rank)), dim3(gat::kMinpThreads), lds, ctx->stream, R);
    else hipLaunchKernelGGL(gat::k_minp_rank<false>, dim3((unsigned)std::min<int64_t>(nb, grid_rank)), dim3(gat::kMinpThreads), lds, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());
    return GAT_OK;
  }
};

extern "C" int gat_minp_counts(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples,
                               const uint8_t* is_double_host, const double* means_host, const int32_t* kobs_host,
                               int64_t* c_out_host) {
  if (!ctx || !counts_dev || !is_double_host || !means_host || !kobs_host || !c_out_host)
    return set_err(ctx, GAT_ERR_ARG, "gat_minp_counts: NULL argument");
  if (n_rows <= 0) return GAT_OK;
  const Knobs kn = read_knobs(ctx);                 // the call's
  { const int rc = MinpRanker::check(ctx, kn, "gat_minp_counts", n_rows, n_samples, kobs_host); if (rc != GAT_OK) return rc; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t S = n_samples;
  // o_1 .. o_R: by (k_obs, row index); proc = that order from its end
  std::vector<int32_t> proc((size_t)n_rows);
  for (int64_t r = 0; r < n_rows; ++r) proc[(size_t)r] = (int32_t)r;
  std::sort(proc.begin(), proc.end(), [&](int32_t a, int32_t b) { return kobs_host[a] != kobs_host[b] ? kobs_host[a] > kobs_host[b] : a > b; });
  std::vector<int32_t> kobs_proc((size_t)n_rows);
  for (int64_t p = 0; p < n_rows; ++p) kobs_proc[(size_t)p] = kobs_host[proc[(size_t)p]];
  DevBuf<int32_t> d_rows, d_kobs, d_q;
  DevBuf<uint32_t> d_c;
  MinpRanker rank;
  HIPCHK(ctx, d_rows.upload(proc, ctx));
  HIPCHK(ctx, d_kobs.upload(kobs_proc, ctx));
  { const int rc = rank.init(ctx, kn, counts_dev, n_rows, n_samples, is_double_host, means_host); if (rc != GAT_OK) return rc; }
  HIPCHK(ctx, d_c.alloc((size_t)n_rows));
  HIPCHK(ctx, d_q.alloc((size_t)S));
  HIPCHK(ctx, hipMemsetAsync(d_c.p, 0, (size_t)n_rows * 4, ctx->stream));
  const bool timed = ctx->kernel_times || kn.kernel_times;
  MinpTimer T;
  ctx->minp_ms[0] = ctx->minp_ms[1] = 0.f;
  if (timed) for (hipEvent_t& e : T.ev) HIPCHK(ctx, hipEventCreate(&e));
  gat::MinpStepArgs Q;
  Q.K = rank.d_K.p; Q.S = (int32_t)S; Q.q = d_q.p;
  const unsigned step_grid = (unsigned)((S + gat::kMinpThreads - 1) / gat::kMinpThreads);
  for (int64_t p0 = 0; p0 < n_rows; p0 += rank.batch) {              // (one stream: a batch's K is read before the next one's is written)
    const int64_t nb = std::min<int64_t>(rank.batch, n_rows - p0);
    if (timed) HIPCHK(ctx, hipEventRecord(T.ev[0], ctx->stream));
    { const int rc = rank.launch(ctx, d_rows.p + p0, nb); if (rc != GAT_OK) return rc; }
    if (timed) HIPCHK(ctx, hipEventRecord(T.ev[1], ctx->stream));
    Q.n_rows = (int32_t)nb; Q.kobs = d_kobs.p + p0; Q.c = d_c.p + p0; Q.first = p0 == 0 ? 1 : 0;
    hipLaunchKernelGGL(gat::k_minp_step, dim3(step_grid), dim3(gat::kMinpThreads), 0, ctx->stream, Q);
    HIPCHK(ctx, hipGetLastError());
    if (timed) { const int rc = T.add(ctx, ctx->minp_ms); if (rc != GAT_OK) return rc; }
  }
  std::vector<uint32_t> c((size_t)n_rows);
  HIPCHK(ctx, staged_d2h(ctx, c.data(), d_c.p, (size_t)n_rows * 4));
  for (int64_t p = 0; p < n_rows; ++p) c_out_host[proc[(size_t)p]] = (int64_t)c[(size_t)p];
  return GAT_OK;
}

extern "C" int gat_minp_times(const gat_ctx* ctx, float* ms_rank, float* ms_step) {
  if (!ctx || !ms_rank || !ms_step) return set_err(nullptr, GAT_ERR_ARG, "gat_minp_times: NULL argument");
  *ms_rank = ctx->minp_ms[0];
  *ms_step = ctx->minp_ms[1];
  return GAT_OK;
}

// The resampling-based FDR's counts (include/gat_mi355.h, gat_efdr.h): the rows are ranked into K in batches as for minP, in
// their own order (V and N are sums over all rows); behind k_minp_rank, k_efdr runs once per chunk of at most
// GAT_EFDR_LDS_THRESHOLDS thresholds over the batch's K.  The 64-bit bins and the per-sample level counts stay on the device
// from batch to batch; the prefix sums over the thresholds are the host's.
extern "C" int gat_efdr_counts(gat_ctx* ctx, const void* counts_dev, int64_t n_rows, int64_t n_samples,
                               const uint8_t* is_double_host, const double* means_host, const int32_t* kobs_host,
                               const int32_t* levels_host, int32_t n_levels, int64_t* v_out_host, int32_t* per_sample_out_host) {
  if (!ctx || !counts_dev || !is_double_host || !means_host || !kobs_host || !v_out_host || (n_levels > 0 && (!levels_host || !per_sample_out_host)))
    return set_err(ctx, GAT_ERR_ARG, "gat_efdr_counts: NULL argument");
  if (n_rows <= 0) return GAT_OK;
  const Knobs kn = read_knobs(ctx);                 // the call's
  { const int rc = MinpRanker::check(ctx, kn, "gat_efdr_counts", n_rows, n_samples, kobs_host); if (rc != GAT_OK) return rc; }
  if (n_levels < 0 || n_levels > gat::kEfdrLevels) return set_err(ctx, GAT_ERR_ARG, "gat_efdr_counts: %d levels (at most %d)", n_levels, gat::kEfdrLevels);
  for (int l = 0; l < n_levels; ++l)
    if (levels_host[l] < 0 || (int64_t)levels_host[l] > n_samples)
      return set_err(ctx, GAT_ERR_ARG, "gat_efdr_counts: level %d is %d of %lld samples", l, levels_host[l], (long long)n_samples);
  const int64_t thr_max = (int64_t)ctx->max_lds / gat::kEfdrThresholdBytes;
  if (kn.efdr_lds_thresholds_set && (kn.efdr_lds_thresholds < 1 || kn.efdr_lds_thresholds > thr_max))
    return set_err(ctx, GAT_ERR_ARG, "gat_efdr_counts: GAT_EFDR_LDS_THRESHOLDS must be in [1, %lld]", (long long)thr_max);
  const int64_t chunk = kn.efdr_lds_thresholds_set ? kn.efdr_lds_thresholds : thr_max;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t S = n_samples;
  std::vector<int32_t> thr(kobs_host, kobs_host + n_rows);          // the sorted distinct k_obs
  std::sort(thr.begin(), thr.end());
  thr.erase(std::unique(thr.begin(), thr.end()), thr.end());
  const int64_t n_thr = (int64_t)thr.size();
  std::vector<int32_t> ident((size_t)n_rows);
  for (int64_t r = 0; r < n_rows; ++r) ident[(size_t)r] = (int32_t)r;
  DevBuf<int32_t> d_rows, d_thr, d_ps;
  DevBuf<unsigned long long> d_bins;
  MinpRanker rank;
  HIPCHK(ctx, d_rows.upload(ident, ctx));
  HIPCHK(ctx, d_thr.upload(thr, ctx));
  { const int rc = rank.init(ctx, kn, counts_dev, n_rows, n_samples, is_double_host, means_host); if (rc != GAT_OK) return rc; }
  HIPCHK(ctx, d_bins.alloc((size_t)(2 * n_thr)));
  HIPCHK(ctx, hipMemsetAsync(d_bins.p, 0, (size_t)(2 * n_thr) * 8, ctx->stream));
  const size_t ps_words = (size_t)n_levels * 2 * (size_t)S;
  HIPCHK(ctx, d_ps.alloc(ps_words));
  if (ps_words) HIPCHK(ctx, hipMemsetAsync(d_ps.p, 0, ps_words * 4, ctx->stream));
  // (the largest chunk's, whatever this call's is: the attribute is the kernel's, and another context's call may be in flight)
  HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_efdr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(thr_max * gat::kEfdrThresholdBytes)));
  const bool timed = ctx->kernel_times || kn.kernel_times;
  MinpTimer T;
  ctx->efdr_ms[0] = ctx->efdr_ms[1] = 0.f;
  if (timed) for (hipEvent_t& e : T.ev) HIPCHK(ctx, hipEventCreate(&e));
  gat::EfdrArgs A;
  A.K = rank.d_K.p; A.counts = (const int64_t*)counts_dev; A.row_stride = S; A.S = (int32_t)S;
  A.is_double = rank.d_dbl.p; A.means = rank.d_means.p; A.bins_stride = n_thr; A.per_sample = d_ps.p;
  const int64_t grid_x = (S + gat::kEfdrThreads - 1) / gat::kEfdrThreads;
  for (int64_t p0 = 0; p0 < n_rows; p0 += rank.batch) {              // (one stream: a batch's K is read before the next one's is written)
    const int64_t nb = std::min<int64_t>(rank.batch, n_rows - p0);
    if (timed) HIPCHK(ctx, hipEventRecord(T.ev[0], ctx->stream));
    { const int rc = rank.launch(ctx, d_rows.p + p0, nb); if (rc != GAT_OK) return rc; }
    if (timed) HIPCHK(ctx, hipEventRecord(T.ev[1], ctx->stream));
    A.n_rows = (int32_t)nb; A.rows = d_rows.p + p0;
    for (int64_t c0 = 0; c0 < n_thr; c0 += chunk) {
      const int64_t nc = std::min<int64_t>(chunk, n_thr - c0);
      // slabs of rows: about eight workgroups per compute unit in all, a slab long enough to pay for a workgroup's pass over
      // its bins (three LDS words and up to two global adds per threshold) and short enough for its 32-bit LDS bins
      // (256 x rows < 2^32), at most 65535 of them (grid y)
      const int64_t slabs_wanted = std::max<int64_t>(1, (2048 + grid_x - 1) / grid_x);
      int64_t rps = std::max<int64_t>((nb + slabs_wanted - 1) / slabs_wanted, (nc + 31) / 32);
      rps = std::min<int64_t>(rps, ((int64_t)1 << 24) - 1);
      rps = std::min<int64_t>(std::max<int64_t>(rps, (nb + 65534) / 65535), nb);
      A.rows_per_slab = (int32_t)rps;
      A.thr = d_thr.p + c0; A.n_thr = (int32_t)nc; A.below = c0 > 0 ? thr[(size_t)c0 - 1] : 0; A.bins = d_bins.p + c0;
      A.n_levels = c0 == 0 ? n_levels : 0;                          // the levels once per batch: with its first chunk
      for (int l = 0; l < gat::kEfdrLevels; ++l) A.levels[l] = l < A.n_levels ? levels_host[l] : -1;
      hipLaunchKernelGGL(gat::k_efdr, dim3((unsigned)grid_x, (unsigned)((nb + rps - 1) / rps)), dim3(gat::kEfdrThreads),
                         (size_t)nc * gat::kEfdrThresholdBytes, ctx->stream, A);
      HIPCHK(ctx, hipGetLastError());
    }
    if (timed) { const int rc = T.add(ctx, ctx->efdr_ms); if (rc != GAT_OK) return rc; }
  }
  std::vector<unsigned long long> bins((size_t)(2 * n_thr));
  HIPCHK(ctx, staged_d2h(ctx, bins.data(), d_bins.p, bins.size() * 8));
  for (int64_t j = 1; j < n_thr; ++j) { bins[(size_t)j] += bins[(size_t)j - 1]; bins[(size_t)(n_thr + j)] += bins[(size_t)(n_thr + j) - 1]; }   // V_d(thr[j])
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t j = std::lower_bound(thr.begin(), thr.end(), kobs_host[r]) - thr.begin();
    v_out_host[2 * r] = (int64_t)bins[(size_t)j];
    v_out_host[2 * r + 1] = (int64_t)bins[(size_t)(n_thr + j)];
  }
  if (ps_words) HIPCHK(ctx, staged_d2h(ctx, per_sample_out_host, d_ps.p, ps_words * 4));
  return GAT_OK;
}

extern "C" int gat_efdr_times(const gat_ctx* ctx, float* ms_rank, float* ms_efdr) {
  if (!ctx || !ms_rank || !ms_efdr) return set_err(nullptr, GAT_ERR_ARG, "gat_efdr_times: NULL argument");
  *ms_rank = ctx->efdr_ms[0];
  *ms_efdr = ctx->efdr_ms[1];
  return GAT_OK;
}
