// gat_types.h -- the records and constants the host side of libgat_mi355.so shares with the kernels: what a host
// translation unit that launches nothing (gat_prep.hip: problem creation, annotation tables) needs to know, without the
// kernels themselves.  Included by gat_device.h / gat_kernels.h / gat_tail.h, which own everything else.
#pragma once
#include <stdint.h>

namespace gat {

constexpr int kWave = 64;
constexpr int kMtN = 624;

constexpr int kWsTreeMin = 32;      // workspaces with more segments get trees (the shorter ones are searched in registers)
constexpr int kWsTreeLevels = 6;   // 16^6 keys; the level loops are unrolled so that the geometry stays in scalar registers

constexpr int kPlaceWsLds = 256;      // k_place: workspace segments kept in LDS (16 B each)
constexpr int kPlaceGridTiles = 8;    // k_place_grid (MODE 5): tiles (waves) of a workgroup around one unit's cdf grid in LDS: two waves per SIMD, each with
                                      // the registers for its look-ups one chunk ahead (rows pinned at v192..v223)
constexpr int kGridHeader = 4;        // words in front of a grid in ws_tree: {shift, cells, widest cell's span, words of the LDS image}
constexpr int kPlaceRankLds = 1024;   // k_place: length-rank table entries kept in LDS
#ifndef GAT_PLACE_WIDE_TILES
#define GAT_PLACE_WIDE_TILES 4         // (tuning builds: -DGAT_PLACE_WIDE_TILES=2 / 8; tools/exp_wide_tiles*.sh: config-4 shape k_place_wide
                                       //  10.7 ms with 8, 9.2 with 4, 11.4 with 2)
#endif
constexpr int kPlaceWide = GAT_PLACE_WIDE_TILES;   // k_place_wide: tiles (waves) of a workgroup, sharing one unit's rank table in LDS
constexpr int kPlaceWideMaxRank = 20480;  // ... whose size is bounded by the LDS beside the eight 8 KB rings (80 KB of 160)
constexpr int kTailMaxWs = 64;        // workspace segments k_tail scans linearly (wave-uniform loop)
constexpr int kMergedSlots = 8;       // k_count_merged: contigs are dealt to this many slots (blockIdx % 8: the XCD stride)
constexpr int kUniverseFixedLdsBytes = 2560;   // k_universe: the generator's state (kMtLdsWords) in front of the mark table

// per isochore unit, everything SamplerAnnotator.sample derives from (segments, workspace) before
// its loop (gat/Engine.pyx:543-565), hoisted to problem creation.
struct UnitDev {
  int32_t n_ws;         // workspace segments of the unit
  int32_t ws_off;       // offset into ws / ws_cdf
  int32_t tree_start_off;  // offset into ws_tree of the search tree over the workspace starts (-1: short workspace)
  int32_t tree_cdf_off;    // ... over the cumulated lengths
  uint32_t hist_total;  // HistogramSampler.total_size == number of working segments
  uint32_t bucket;      // bucket size (after the bucket_size==0 rule, gat/SegmentList.pyx:1164)
  uint32_t ws_total;    // SegmentListSampler.total_size == workspace bases
  int32_t ltotal;       // bases to reproduce (gat/Engine.pyx:550-552)
  int32_t slab_off;     // offset of the unit's output region inside a sample's slab
  int32_t slab_cap;     // capacity of that region == LDS buffer capacity used for the unit
  int32_t contig;
  int32_t rank_off;     // offset into rank_len: rank_len[r] = bucket index searchsorted(cdf, r) returns
  int32_t n_target;     // SamplerSegments: len(segments) placements (gat/Engine.pyx:726)
  int32_t pad;          // units_o: the unit id
  // fragmented workspaces (round 6; both -1 for a short workspace), offsets into ws_tree, kGridHeader words in front of each:
  int32_t pgrid_off;    // position grid: entry c = the first workspace segment whose END lies beyond c << shift (u32 entries;
                        //   cells + 1 of them, the last = n_ws): the overlap of [s, e) with the workspace is a walk from entry s >> shift
  int32_t cgrid_off;    // grid over the cumulated lengths (the position draw's searchsorted, gat/Engine.pyx:299-305): u16 entries
                        //   g[c] = #{i : cdf[i] < c << shift} (cells + 1, padded to a word), then u16 keys cdf[i] & ((1 << shift) - 1):
                        //   #{cdf < p} = g[c] + #{i in [g[c], g[c + 1]) : key[i] < (p & mask)} for c = p >> shift -- the image k_place_grid
                        //   copies into LDS (2 bytes per workspace segment + 2 per cell)
};
static_assert(sizeof(UnitDev) == 64, "UnitDev: sixteen words");

enum : int32_t {
  kStatusOverflow = 1,   // LDS/slab capacity exceeded: host retries with a larger slab
  kStatusAssert = 2,     // reference assert would fire (gat/Engine.pyx:645 sum()>0)
  kStatusTrimAssert = 4, // gat/SegmentList.pyx:560 sum() > size
  kStatusUnitsOverlap = 16, // k_units_overlap: overlaps between the units' lists that are not pairwise (or more candidates than the
                         // buffer holds): host repeats the batch through k_contig and keeps to it for the problem
  kStatusCoordRange = 32, // k_permute_local: a start or end of the walk beyond 2^31 - 1, where the reference's assignment to its C int
                         // raises OverflowError (gat/Engine.pyx:1208, :1212)
  // (SamplerBruteForce's "sampling did not converge" is no status bit: it is counted, and the first such work unit named, in
  //  the batch's statistics words -- gat_brute_force.h)
  kStatusContigLds = 8,  // k_contig: a contig's lists exceed the LDS the launch was given (sized for what is expected,
                         // not for every unit at its capacity): host repeats the batch with the full size
};

// The status block of a sampler batch: kStatSlotWords 64-bit words on the device (gat_problem::d_stat), mirrored per batch in a
// pinned slot (gat_ctx::h_stat, CallBlock::stat_slot).  The host zeroes words [0, kStatCopied) in front of a batch's kernels and
// copies them into the slot behind them; the words beyond have an owner each that zeroes / copies its own.  This is the one place
// that says what a word means: kernels and host refer to the names.
enum : int {
  // k_reduce_stats, summed over the batch's work units (contiguous from 0: it stores them as stat[threadIdx.x])
  kStatPlaced = 0,         // segments placed
  kStatDraws = 1,          // draws
  kStatUnsuccessful = 2,   // unsuccessful rounds
  kStatTailUnits = 3,      // work units finished by k_tail / carried on by k_tail_big
  kStatFullUnits = 4,      // work units k_sampler ran in full
  kStatResumedUnits = 5,   // work units k_sampler resumed with a stream moved up
  kStatReduced = 6,        // (their number)
  kStatRestarts = 6,       // k_brute_force: restarts + (work units not converged << kBruteUnconvShift)
  kStatEmptyWindows = 7,   // k_shift: segments with an empty window
  kStatFlags = 8,          // int32, OR of kStatus*: every sampler kernel, through gat_problem::flags_dev()
  kStatQueued = 9,         // uint32, k_tail's queue length: through gat_problem::todo_count_dev()
  kStatCopied = 10,        // words [0, kStatCopied): zeroed and copied per batch
  kStatUnitsOverlap = 10,  // PINNED SLOT ONLY, kStatUnitsOverlapWords words: k_units_overlap's four 32-bit words {status (bit 0: not
                           // pairwise; else a candidate region overflowed), overlaps taken off, candidates, free}, copied from
                           // d_cand_count + kCandSlots behind the count kernels or zeroed by the host
  kStatUnitsOverlapWords = 2,
  kStatBruteFirst = 12,    // k_brute_force: ~((sample << 32) | unit) of the first work unit that did not converge (atomicMax);
                           // zeroed and copied by the brute-force stage alone
  kStatDbgWhy = 10,        // DEVICE ONLY, -DGAT_DBG_QUEUE builds only, kStatDbgWhyWords words: k_tail's counters of why a round was
                           // broken (such a build zeroes and prints the whole slot)
  kStatDbgWhyWords = 6,
  kStatSlotWords = 16,
};
static_assert(kStatPlaced == 0 && kStatDraws == 1 && kStatUnsuccessful == 2 && kStatTailUnits == 3 && kStatFullUnits == 4 &&
              kStatResumedUnits == 5 && kStatReduced == 6, "k_reduce_stats stores its six sums as stat[threadIdx.x]");
static_assert(kStatReduced <= kStatRestarts && kStatRestarts < kStatCopied && kStatEmptyWindows < kStatCopied &&
              kStatFlags < kStatCopied && kStatQueued < kStatCopied, "the words every batch zeroes and copies");
static_assert(kStatCopied <= kStatUnitsOverlap, "the batch's copy must not overwrite k_units_overlap's words in the pinned slot");
static_assert(kStatUnitsOverlap + kStatUnitsOverlapWords <= kStatBruteFirst, "k_units_overlap's words end before k_brute_force's");
static_assert(kStatBruteFirst < kStatSlotWords && kStatDbgWhy >= kStatCopied && kStatDbgWhy + kStatDbgWhyWords <= kStatSlotWords,
              "everything fits in the slot");

}  // namespace gat
