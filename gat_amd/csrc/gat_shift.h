// gat_shift.h -- SamplerShift (gat/Engine.pyx:998-1111) on the device: k_shift, one wave per (sample, unit).
//
// Per work unit the stream is the per-unit one of every sampler here (numpy.random.seed((seed + sample*n_units + unit)
// mod 2^32)), run by the wave's in-LDS MT19937 (WaveRng).  The unit's working segments are walked in order;
// each one's window -- the workspace pieces within `area` of its midpoint, truncated -- was laid down at problem creation
// (gat_prep_units.h: shift_windows) as a run [lo, lo + k) of the unit's workspace with its first start and last end clipped,
// so the position draw is a search of the workspace cdf restricted to the run and the fills walk the run.  The pieces go
// to the unit's slab region as they come; the list is then sorted and merged with SegmentList.normalize's rule (overlaps
// united, adjacent pieces kept apart: gat/SegmentList.pyx:697-750) -- in LDS when it fits, in the slab otherwise.
//
// The reference's integer types are kept throughout: Position uint32, PositionDifference int32, lmin / lmax signed
// (gat/SegmentList.pxd:31-33, gat/SegmentList.pyx:68-77).  tests/shift_model.py is the same walk in Python.
#pragma once
#include "gat_kernels.h"

namespace gat {

struct ShiftArgs {
  const UnitDev* units_o;     // active units in launch order, unit id in `pad`
  int32_t n_units;
  int32_t n_active;
  int32_t rec_stride;         // ws_stat: [unit][rec_stride]
  int32_t lds_cap;            // segments the LDS list buffer holds
  const uint2* ws;
  const uint32_t* ws_cdf;     // cumulated lengths - 1, per unit
  const uint4* shift;         // two records per working segment (gat_problem::d_shift)
  const int32_t* shift_off;   // per unit: first record pair
  uint32_t seed;
  int64_t sample_begin;
  uint2* slab;
  int64_t slab_stride;
  int32_t* unit_n;            // [batch][n_units]
  int32_t* flags;
  unsigned long long* stat;   // the batch's status block: kStatEmptyWindows (gat_types.h)
  uint32_t* ws_stat;
};

__device__ __forceinline__ int32_t shift_lmin(int32_t a, int32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t shift_lmax(int32_t a, int32_t b) { return a > b ? a : b; }

__global__ __launch_bounds__(64) void k_shift(ShiftArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int sidx = (int)blockIdx.x;
  const int a = (int)(blockIdx.y + blockIdx.z * gridDim.y);
  if (a >= A.n_active) return;
  const UnitDev U = A.units_o[a];
  const int u = U.pad;
  const uint2* __restrict__ ws = A.ws + U.ws_off;
  const uint32_t* __restrict__ cdf = A.ws_cdf + U.ws_off;
  const uint4* __restrict__ rec = A.shift + 2 * (int64_t)A.shift_off[u];
  uint2* out = A.slab + (int64_t)sidx * A.slab_stride + U.slab_off;
  const int cap = U.slab_cap;
  const int nwork = (int)U.hist_total;
  const uint32_t seed = unit_stream_seed(A.seed, A.sample_begin, sidx, A.n_units, u);

  WaveRng rng;
  rng.mt = lds;
  rng_seed(rng, seed, lane);
  rng_no_rows(rng); rng.seed = seed;

  int nout = 0;
  int status = 0;
  uint32_t empty = 0;
  // (wave-uniform control flow: every lane walks the same segment; lane 0 stores the pieces)
  auto emit = [&](uint32_t s, uint32_t e) {
    if (nout < cap) { if (lane == 0) out[nout] = make_uint2(s, e); }
    else status |= kStatusOverflow;
    nout++;
  };

  for (int i = 0; i < nwork; ++i) {
    const uint4 r0 = rec[2 * i], r1 = rec[2 * i + 1];
    const uint32_t length = r0.x, lo = r0.y, sum = r0.w, fs = r1.x, le = r1.y;
    const int k = (int)r0.z;
    auto piece = [&](int j) -> uint2 {
      uint2 p = ws[lo + (uint32_t)j];
      if (j == 0) p.x = fs;
      if (j == k - 1) p.y = le;
      return p;
    };
    // SegmentList.getInsertionPoint(x, x + 1) on the window with its border cases (-1 -> 0, n -> n - 1): the last piece
    // starting at or before x, the first one for x before the window, the last one for x at or beyond its end
    auto ins = [&](uint32_t x) -> int {
      if (x >= le) return k - 1;
      if (x < fs) return 0;
      int l = 1, h = k;                                    // first piece j >= 1 with start > x
      while (l < h) {
        const int m = (l + h) >> 1;
        if (ws[lo + (uint32_t)m].x > x) h = m; else l = m + 1;
      }
      return l - 1;
    };
    // getFilledSegmentsFromStart / FromEnd (gat/SegmentList.pyx:1314-1399): wrap round the window; all of it when the
    // remainder exceeds its bases.  (The bound on the steps is a guard only: the reference's loop ends within two turns.)
    auto fill_all = [&]() {
      for (int j0 = 0; j0 < k; j0 += kWave) {
        const int j = j0 + lane;
        if (nout + j < cap && j < k) out[nout + j] = piece(j);
      }
      if (nout + k > cap) status |= kStatusOverflow;
      nout += k;
    };
    auto fill_start = [&](uint32_t x, int32_t rem) {
      if ((uint32_t)rem > sum) { fill_all(); return; }
      if (rem <= 0) return;
      int idx = ins(x);
      uint32_t start = x;
      for (int guard = 0; rem > 0; ++guard) {
        if (guard > 4 * k + 8) { status |= kStatusAssert; break; }
        const uint2 p = piece(idx);
        if (!(p.y < start)) {
          start = (uint32_t)shift_lmax((int32_t)p.x, (int32_t)start);
          const uint32_t end = (uint32_t)shift_lmin((int32_t)p.y, (int32_t)(start + (uint32_t)rem));
          rem = (int32_t)((uint32_t)rem - (end - start));
          emit(start, end);
        }
        if (++idx == k) { idx = 0; start = piece(0).x; }
      }
    };
    auto fill_end = [&](uint32_t x, int32_t rem) {
      if ((uint32_t)rem > sum) { fill_all(); return; }
      if (rem <= 0) return;
      int idx = ins(x);
      uint32_t end = x;
      for (int guard = 0; rem > 0; ++guard) {
        if (guard > 4 * k + 8) { status |= kStatusAssert; break; }
        const uint2 p = piece(idx);
        if (!(p.x > end)) {
          end = (uint32_t)shift_lmin((int32_t)p.y, (int32_t)end);
          const uint32_t start = (uint32_t)shift_lmax((int32_t)p.x, (int32_t)(end - (uint32_t)rem));
          rem = (int32_t)((uint32_t)rem - (end - start));
          emit(start, end);
        }
        if (--idx < 0) { idx = k - 1; end = piece(k - 1).y; }
      }
    };

    // getRandomPosition (gat/SegmentList.pyx:902-917): randint(0, sum), then the walk with `pos > l` (pos == l is that
    // piece's end).  An empty window: randint(0, 0) raises inside the cpdef, which returns 0 -- no draw.
    int32_t start;
    if (sum == 0) {
      start = 0;
      empty++;
    } else {
      uint32_t pos = rng_range(rng, sum - 1u, lane);
      const uint32_t l0 = (k == 1 ? le : ws[lo].y) - fs;
      if (pos <= l0) {
        start = (int32_t)(fs + pos);
      } else {
        pos -= l0;
        const uint32_t c0 = cdf[lo];
        int l = 1, h = k - 1;                              // first j in [1, k - 1) with C(j) >= pos, else k - 1
        while (l < h) {
          const int m = (l + h) >> 1;
          if (cdf[lo + (uint32_t)m] - c0 >= pos) h = m; else l = m + 1;
        }
        start = (int32_t)(ws[lo + (uint32_t)l].x + pos - (cdf[lo + (uint32_t)l - 1u] - c0));
      }
    }
    int32_t end;
    if (rng_range(rng, 1u, lane)) {
      end = (int32_t)((uint32_t)start + length);
    } else {
      end = start;
      start = (int32_t)((uint32_t)end - length);
    }
    const int32_t wss = k ? (int32_t)fs : 0, wse = k ? (int32_t)le : 0;       // ws.min(), ws.max() (0 when empty)
    if (start < wss) {
      const int32_t rem = shift_lmin((int32_t)((uint32_t)wss - (uint32_t)start), (int32_t)length);
      fill_start((uint32_t)start, (int32_t)(length - (uint32_t)rem));
      fill_end((uint32_t)wse, rem);
    } else if (end > wse) {
      const int32_t rem = shift_lmin((int32_t)((uint32_t)end - (uint32_t)wse), (int32_t)length);
      fill_end((uint32_t)end, (int32_t)(length - (uint32_t)rem));
      fill_start((uint32_t)wss, rem);
    } else {
      fill_start((uint32_t)start, (int32_t)length);
    }
  }

  // sample.normalize(): sort by start, unite overlaps, keep adjacent pieces apart, drop empties
  int n = status ? 0 : nout;
  __syncthreads();                                        // (lane 0's stores to the slab, seen by the wave)
  if (n > 1) {
    if (n <= A.lds_cap) {
      uint2* seg = reinterpret_cast<uint2*>(lds + kMtLdsWords);
      for (int j = lane; j < n; j += kWave) seg[j] = out[j];
      wave_sort_auto(seg, n, lane);
      n = wave_merge0<false, true>(seg, n, lane);
      for (int j = lane; j < n; j += kWave) out[j] = seg[j];
    } else {
      wave_sort_by_start<true>(out, n, lane);
      n = wave_merge0<true, true>(out, n, lane);
    }
  } else if (n == 1 && out[0].x == out[0].y) {
    n = 0;
  }
  if (lane == 0) {
    A.unit_n[(int64_t)sidx * A.n_units + u] = n;
    if (status) atomicOr(A.flags, status);
    *reinterpret_cast<uint4*>(A.ws_stat + ((int64_t)u * A.rec_stride + sidx) * 4) = make_uint4((uint32_t)nwork, rng.ndraws, 0u, 1u);
    if (empty) atomicAdd(&A.stat[kStatEmptyWindows], (unsigned long long)empty);
  }
}

}  // namespace gat
