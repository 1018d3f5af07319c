// gat_annotator_steps.h -- the steps of SamplerAnnotator.sample's loop (gat/Engine.pyx:572-646), each held once for every
// kernel that walks it: k_sampler / k_serial (sampler_unit), k_tail, k_tail_big, k_resume_big and the list samplers.
// Nothing here knows which kernel calls it.  The first part is plain code for host and device -- no intrinsic, no runtime
// call -- so that it runs (and is checked: tests/host/annotator_steps_check.cpp) without a device; the second part is the
// same loop's steps done by one wave over a list of segments.
#pragma once
#include <stdint.h>
#include "gat_device.h"

namespace gat {

// ---- plain steps ------------------------------------------------------------------------------------------------

// The stream of work unit (sample, unit): numpy.random.seed((seed + sample * n_units + unit) mod 2^32), `sample` counted over
// the whole run (DESIGN section 2's contract: a result does not depend on how a run is cut into batches)
__host__ __device__ __forceinline__ uint32_t unit_stream_seed(uint32_t seed, int64_t sample_begin, int64_t sidx, int32_t n_units, int32_t u) {
  const uint64_t sample_id = (uint64_t)(sample_begin + sidx);
  return (uint32_t)((uint64_t)seed + sample_id * (uint64_t)n_units + (uint64_t)u);
}

// SegmentListSampler.sample (gat/Engine.pyx:299-343) behind the choice of the workspace piece [cs, ce): a segment of `length`
// bases that overlaps the piece starts in [cs - length + 1, ce), the lower end clamped to the end of the piece in front
// (prev_end, kNoPieceInFront for the first piece; the reference's int32 lmax) -- the offset is drawn from [0, range] ...
constexpr int32_t kNoPieceInFront = INT32_MIN;
struct PlaceRange { int32_t sampling_start; uint32_t range; };
__host__ __device__ __forceinline__ PlaceRange place_range(uint32_t cs, uint32_t ce, int32_t prev_end, int32_t length) {
  int32_t sampling_start = (int32_t)cs - length + 1;
  sampling_start = prev_end > sampling_start ? prev_end : sampling_start;
  return {sampling_start, ce - 1u - (uint32_t)sampling_start};
}
// ... and q = sampling_start + offset gives the segment [max(0, q), q + length) and the bases of it inside the piece.
// The domain (gat_problem_create refuses a unit outside it: unit_lmax, gat_prep_units.h): ce + length - 1 <= 2^31 - 1, so
// q + length <= 2^31 - 1 for every q a placement can draw (q <= ce - 1), and q + length >= 1 (q >= cs - length + 1).  No
// signed operation here can overflow inside it: the end is an unsigned sum, the overlap an unsigned difference of two
// values below 2^31.
struct Placed { uint32_t start, end; int32_t overlap; };
__host__ __device__ __forceinline__ Placed place_at(uint32_t cs, uint32_t ce, int32_t q, int32_t length) {
  const uint32_t start = (uint32_t)(q > 0 ? q : 0);
  const uint32_t end = (uint32_t)q + (uint32_t)length;
  const int32_t omin = (int32_t)ce < (int32_t)end ? (int32_t)ce : (int32_t)end;
  const int32_t omax = (int32_t)cs > (int32_t)start ? (int32_t)cs : (int32_t)start;
  const int32_t overlap = (int32_t)((uint32_t)omin - (uint32_t)omax);
  return {start, end, overlap > 0 ? overlap : 0};
}

// HistogramSampler.sample (gat/Engine.pyx:413-435) on the unit's compressed cdf: rank_len[r] is the bucket searchsorted(cdf, r)
// returns (tabulated per rank at problem creation); one draw, a second one inside the bucket when bucket > 1.
// draw(range): uniform in [0, range] from the unit's stream.
template <class Draw>
__host__ __device__ __forceinline__ uint32_t length_draw(uint32_t hist_total, const uint32_t* __restrict__ rank_len, uint32_t bucket,
                                                         Draw draw) {
  uint32_t r = 1;
  if (hist_total > 1) r = 1u + draw(hist_total - 2u);
  uint32_t len_u = rank_len[r] * bucket;
  if (bucket > 1) len_u += draw(bucket - 1u);
  return len_u;
}

// The bookkeeping behind a consolidation (gat/Engine.pyx:601-605) -- a round that did not change what is left to cover counts
// as unsuccessful -- and the loop's test behind it: false when nothing is left or kMaxUnsuccessful rounds went without progress
constexpr int kMaxUnsuccessful = 20;
__host__ __device__ __forceinline__ bool consolidate_progress(int32_t remaining, int32_t& true_remaining, int& nuns) {
  if (true_remaining == remaining) nuns++; else true_remaining = remaining;
  return true_remaining != 0 && nuns < kMaxUnsuccessful;
}

// SegmentList.trim_ends(pos, s, forward) (gat/SegmentList.pyx:545-597) from element k of n (k = _getInsertionPoint(pos, pos + 1)):
// s bases are taken off the list, whole elements emptied to [0, 0), the last one shortened at its front (forward) or its
// back, walking round the list's end.  at(i): element i, by reference; overlap(a, b): the workspace bases in [a, b).
// The caller has made sure that the list holds more than s bases.  One thread's work.
struct TrimWalk {
  uint32_t removed;   // workspace bases the trim took away
  int last;           // the element it shortened last (emptied where its length was what remained of s), -1: s <= 0
};
template <class At, class Overlap>
__host__ __device__ __forceinline__ TrimWalk trim_ends_walk(int n, int k, int32_t s, bool forward, At at, Overlap overlap) {
  TrimWalk r = {0u, -1};
  int idx = k;
  while (s > 0) {
    uint2& el = at(idx);
    const uint2 v = el;
    const int32_t l = (int32_t)v.y - (int32_t)v.x;
    uint32_t ra, rb;                       // removed range
    if (l < s) { el = make_uint2(0u, 0u); s -= l; ra = v.x; rb = v.y; }
    else {
      if (forward) { el = make_uint2(v.x + (uint32_t)s, v.y); ra = v.x; rb = v.x + (uint32_t)s; }
      else { el = make_uint2(v.x, (uint32_t)((int32_t)v.y - s)); ra = (uint32_t)((int32_t)v.y - s); rb = v.y; }
      s = 0;
      r.last = idx;
    }
    if (rb > ra) r.removed += overlap(ra, rb);
    if (forward) { idx++; if (idx == n) idx = 0; }
    else { idx--; if (idx < 0) idx = n - 1; }
  }
  return r;
}

// ---- one wave's steps -------------------------------------------------------------------------------------------

// A stream that comes from the in-LDS generator alone (no rows of k_rng's)
__device__ __forceinline__ void rng_no_rows(WaveRng& r) { r.pre = nullptr; r.pre_j = 0; r.pre_rows = 0; r.pre_base = 0; }

// ... and one that goes on at output `ndraws` of sample sidx's column of the unit's rows (k_rng: tiles of 64 samples, `rows`
// outputs each, the unit's first tile at rng_out + off).  can_switch / seed / mt are the caller's.  rng_rows_at: the same
// rows from another output on.
__device__ __forceinline__ void rng_rows_at(WaveRng& r, uint32_t ndraws) {
  r.ndraws = ndraws; r.pre_j = r.ndraws; r.pre_base = r.pre_j - (uint32_t)kWave;     // (forces the first prefetch)
}
__device__ __forceinline__ void rng_open_rows(WaveRng& r, const uint32_t* rng_out, int64_t off, uint32_t rows, int sidx, uint32_t ndraws) {
  r.use_pre = true; r.exhausted = false; r.pos = 0; r.rbuf = 0;
  r.pre_rows = rows;
  rng_rows_at(r, ndraws);
  r.pre = rng_out + off + (int64_t)(sidx >> 6) * r.pre_rows * kWave + (sidx & 63);
}

__device__ __forceinline__ uint32_t hist_sample(WaveRng& rng, uint32_t hist_total, const uint32_t* __restrict__ rank_len,
                                                uint32_t bucket, int lane) {
  return length_draw(hist_total, rank_len, bucket, [&](uint32_t range) -> uint32_t { return rng_range(rng, range, lane); });
}

// The piece of the workspace that holds base p (searchsorted over the cumulated lengths with cmpPosition, utils/gat_utils.c:36)
// and the end of the piece in front of it.  in_regs: the workspace is W (lane i = piece i): one compare per lane; else
// bisect(p) finds it and ws holds it.
struct WsPiece { uint2 piece; int32_t prev_end; int k; };
template <class Bisect>
__device__ __forceinline__ WsPiece ws_pick(const WsRegs& W, int nws, bool in_regs, const uint2* __restrict__ ws, uint32_t p, int lane,
                                           Bisect bisect) {
  WsPiece r;
  r.prev_end = kNoPieceInFront;
  if (in_regs) {
    const uint64_t b = __ballot(lane < nws && (int32_t)(W.cdf - p) >= 0);
    r.k = (int)__builtin_ctzll(b);
    r.piece.x = (uint32_t)__builtin_amdgcn_readlane((int)W.start, r.k);
    r.piece.y = (uint32_t)__builtin_amdgcn_readlane((int)W.end, r.k);
    if (r.k > 0) r.prev_end = __builtin_amdgcn_readlane((int)W.end, r.k - 1);
  } else {
    r.k = bisect(p);
    r.piece = ws[r.k];
    if (r.k > 0) r.prev_end = (int32_t)ws[r.k - 1].y;
  }
  return r;
}

// SegmentListSampler.sample (gat/Engine.pyx:299-328) over a workspace in memory: a base of the workspace, the piece k that
// holds it, the offset.  Returns random_pos_in_segment; the segment is [max(0, q), q + length).
template <typename Bisect>
__device__ __forceinline__ int32_t ws_sample(WaveRng& rng, const uint2* __restrict__ ws, uint32_t ws_total, int32_t length,
                                             Bisect bisect, int lane, int& k) {
  const uint32_t p = rng_range(rng, ws_total - 1u, lane);
  k = bisect(p);
  const uint2 chosen = ws[k];
  const PlaceRange pr = place_range(chosen.x, chosen.y, k > 0 ? (int32_t)ws[k - 1].y : kNoPieceInFront, length);
  return pr.sampling_start + (int32_t)rng_range(rng, pr.range, lane);
}

// intersect(workspace).sum() and sum() of seg[0, n): the lane's shares, R segments per lane whose workspace searches run
// interleaved
template <int R, class Overlap>
__device__ __forceinline__ void list_coverage(const uint2* seg, int n, int lane, Overlap overlap, uint32_t& lane_cov, uint32_t& lane_tot) {
  for (int base = 0; base < n; base += R * kWave) {
    uint2 v[R];
    uint32_t ov[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = base + r * kWave + lane;
      v[r] = i < n ? seg[i] : make_uint2(0u, 0u);
      lane_tot += v[r].y - v[r].x;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) ov[r] = overlap(v[r].x, v[r].y);
#pragma unroll
    for (int r = 0; r < R; ++r) lane_cov += ov[r];
  }
}

}  // namespace gat
