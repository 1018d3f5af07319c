// gat_brute_force.h -- SamplerBruteForce (gat/Engine.pyx:746-871) on the device: k_brute_force, one wave per (sample, unit).
//
// Per work unit the stream is the per-unit one of every sampler here (numpy.random.seed((seed + sample*n_units + unit)
// mod 2^32)), run by the wave's in-LDS MT19937 (WaveRng).  The sampler is SamplerAnnotator's rejection
// counterpart: a length from the unit's histogram (hist_sample) and a position in the workspace (ws_sample) -- the draws
// k_sampler makes, through the same two functions -- give a segment [max(0, q), q + length) and its overlap with the CHOSEN
// workspace piece; the segment is accepted when that overlap does not exceed `remaining` and the segment overlaps no
// accepted one by a base (touching is no overlap).  An accepted segment takes its overlap off `remaining`, which starts at
// segments.sum() -- over ALL of the unit's segments, as the int32 the reference forms (UnitDev::ltotal) -- and puts the
// tries left back to ntries_inner; a rejected one costs a try.  A pass that ends with tries left has converged (remaining
// <= 0).  Otherwise the list is dropped and the next pass begins where the stream stands; after ntries_outer passes the unit
// has not converged: its status record says so, the call fails with the reference's ValueError.
//
// The accepted list is kept in the order of acceptance: entries [0, lds_cap) in LDS, the ones beyond at their own index in
// the unit's slab region.  The overlap test runs across the lanes, 64 accepted segments per step, a ballot per step; the
// reference's sample.normalize() behind every acceptance is a sort (nothing overlaps, so nothing merges, and adjacent
// segments stay apart), done once at the end with SegmentList.normalize's rule -- in LDS when the list fits, in the slab
// otherwise.  The list is not clipped to the workspace.  A list that outgrows the unit's region sets kStatusOverflow: the
// batch is repeated with doubled regions from the same seeds.
//
// The reference's integer types are kept: remaining / overlap int32 (PositionDifference), lmin / lmax signed
// (gat/SegmentList.pyx:68-77), the position draw's lower end an int32 maximum.  tests/brute_force_model.py is the same
// loop in Python.
#pragma once
#include "gat_kernels.h"
#include "gat_shift.h"

namespace gat {

struct BruteForceArgs {
  const UnitDev* units_o;     // active units in launch order, unit id in `pad`
  int32_t n_units;
  int32_t n_active;
  int32_t rec_stride;         // ws_stat: [unit][rec_stride]
  int32_t lds_cap;            // accepted segments the LDS list buffer holds
  int32_t ntries_inner;
  int32_t ntries_outer;
  const uint2* ws;
  const uint32_t* ws_cdf;     // cumulated lengths - 1, per unit
  const uint32_t* rank_len;
  uint32_t seed;
  int64_t sample_begin;
  uint2* slab;
  int64_t slab_stride;
  int32_t* unit_n;            // [batch][n_units]
  int32_t* flags;
  unsigned long long* stat;   // the batch's status block: kStatRestarts, kStatBruteFirst (gat_types.h)
  uint32_t* ws_stat;
};

constexpr int kBruteLdsCap = 256;          // accepted segments in LDS: 2 KB beside the generator's 2.5
constexpr int kBruteUnconvShift = 40;     // kStatRestarts: the restarts below this bit, the work units not converged from it up

__global__ __launch_bounds__(64) void k_brute_force(BruteForceArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int sidx = (int)blockIdx.x;
  const int a = (int)(blockIdx.y + blockIdx.z * gridDim.y);
  if (a >= A.n_active) return;
  const UnitDev U = A.units_o[a];
  const int u = U.pad;
  const int nws = U.n_ws;
  const uint2* __restrict__ ws = A.ws + U.ws_off;
  const uint32_t* __restrict__ cdf = A.ws_cdf + U.ws_off;
  const uint32_t* __restrict__ rank_len = A.rank_len + U.rank_off;
  uint2* out = A.slab + (int64_t)sidx * A.slab_stride + U.slab_off;
  const int cap = U.slab_cap;
  const int lcap = A.lds_cap;
  const uint64_t sample_id = (uint64_t)(A.sample_begin + sidx);
  const uint32_t seed = unit_stream_seed(A.seed, A.sample_begin, sidx, A.n_units, u);

  WaveRng rng;
  rng.mt = lds;
  rng_seed(rng, seed, lane);
  rng_no_rows(rng); rng.seed = seed;
  uint2* list = reinterpret_cast<uint2*>(lds + kMtLdsWords);
  auto ws_bisect = [&](uint32_t p) -> int { return bisect_u32(cdf, nws, p); };

  int n = 0, status = 0, passes = 0;
  uint32_t placed = 0, rejected = 0;
  bool converged = false;
  // (wave-uniform control flow: every lane draws the same segment; lane 0 stores it)
  for (int outer = A.ntries_outer; outer > 0 && !status; --outer) {
    ++passes;
    n = 0;                                                 // sample.clear(): the stream goes on
    int32_t remaining = U.ltotal;
    int inner = A.ntries_inner;
    while (remaining > 0 && inner > 0) {
      const int32_t length = (int32_t)hist_sample(rng, U.hist_total, rank_len, U.bucket, lane);
      int k;
      const int32_t q = ws_sample(rng, ws, U.ws_total, length, ws_bisect, lane, k);
      const uint2 chosen = ws[k];
      const uint32_t start = (uint32_t)(q > 0 ? q : 0), end = (uint32_t)(q + length);
      // range_overlap(chosen, [start, end)) (gat/SegmentList.pyx:99-103)
      const int32_t ov_raw = shift_lmin((int32_t)chosen.y, (int32_t)end) - shift_lmax((int32_t)chosen.x, (int32_t)start);
      const int32_t overlap = ov_raw > 0 ? ov_raw : 0;
      bool reject = overlap > remaining;
      // sample.overlapWithRange(start, end) != 0: some accepted segment shares a base with it
      for (int base = 0; base < n && !reject; base += kWave) {
        const int i = base + lane;
        bool hit = false;
        if (i < n) {
          const uint2 v = i < lcap ? list[i] : out[i];
          hit = shift_lmin((int32_t)v.y, (int32_t)end) - shift_lmax((int32_t)v.x, (int32_t)start) > 0;
        }
        reject = __ballot(hit) != 0ull;
      }
      if (reject) { --inner; ++rejected; continue; }
      if (n >= cap) { status |= kStatusOverflow; break; }
      if (n < lcap) {
        if (lane == 0) list[n] = make_uint2(start, end);
        wave_sync();
      } else {
        if (lane == 0) out[n] = make_uint2(start, end);
        wave_sync<true>();                                 // (lane 0's store to the slab, seen by the wave)
      }
      ++n;
      ++placed;
      inner = A.ntries_inner;
      remaining -= overlap;
    }
    if (inner > 0) { converged = !status; break; }
  }

  // sample.normalize(): sort by start, adjacent segments kept apart (nothing overlaps, nothing is empty)
  n = converged ? n : 0;
  if (n <= lcap) {
    if (n > 1) {
      wave_sort_auto(list, n, lane);
      n = wave_merge0<false, true>(list, n, lane);
    }
    for (int j = lane; j < n; j += kWave) out[j] = list[j];
  } else {
    for (int j = lane; j < lcap; j += kWave) out[j] = list[j];
    __syncthreads();
    wave_sort_by_start<true>(out, n, lane);
    n = wave_merge0<true, true>(out, n, lane);
  }
  if (lane == 0) {
    A.unit_n[(int64_t)sidx * A.n_units + u] = n;
    if (status) atomicOr(A.flags, status);
    *reinterpret_cast<uint4*>(A.ws_stat + ((int64_t)u * A.rec_stride + sidx) * 4) = make_uint4(placed, rng.ndraws, rejected, 1u);
    if (!status) {
      const unsigned long long unconv = converged ? 0ull : 1ull;
      if (passes > 1 || unconv) atomicAdd(&A.stat[kStatRestarts], (unsigned long long)(passes - 1) + (unconv << kBruteUnconvShift));
      if (unconv) atomicMax(&A.stat[kStatBruteFirst], ~((sample_id << 32) | (unsigned long long)(uint32_t)u));
    }
  }
}

}  // namespace gat
