// gat_circular.h -- SamplerCircular on the device: k_circular, one wave per (sample, unit).  The reference has no such
// sampler; the contract is DESIGN.md section 5 ("k_circular") and tests/circular_model.py is the same in Python.
//
// Per work unit the stream is the per-unit one of every sampler here (numpy.random.seed((seed + sample*n_units + unit)
// mod 2^32)), run by the wave's in-LDS MT19937.  Problem creation (gat_prep_units.h: circular_intervals) laid
// down the working list -- the unit's segments cut to the workspace W -- in linear workspace coordinates: n sorted,
// disjoint, non-touching intervals {a, length}.  One draw, r = randint(0, Wsum); interval x then covers the linear range
// [a_x + r, a_x + r + length_x) of W modulo Wsum.  As in k_permute's second half the ranges are taken in the doubled
// workspace: a counting pass gives the pieces per interval (one, and one more per border of W or wrap it crosses) and how
// many lie beyond the wrap, the writing pass puts every piece at its rotated place -- the pieces at linear positions
// >= Wsum come first in genome order.  Nothing is united: the pieces are disjoint, and touching ones stay apart.  At most
// n + |W| pieces, the unit's slab capacity.
//
// Linear positions reach 2 Wsum < 2^33: 64 bits.  Genome coordinates are uint32.  No list in LDS and no sort: the LDS is
// the generator's state alone.
#pragma once
#include "gat_kernels.h"

namespace gat {

struct CircularArgs {
  const UnitDev* units_o;     // active units in launch order, unit id in `pad`
  int32_t n_units;
  int32_t n_active;
  int32_t rec_stride;         // ws_stat: [unit][rec_stride]
  const uint2* ws;            // W: the unit's workspace pieces at UnitDev::ws_off
  const uint32_t* ws_cdf;     // cumulated lengths - 1, per unit
  const uint4* circ_unit;     // per unit {intervals offset, n, |W|, Wsum}
  const uint2* circ_iv;       // the working list in linear coordinates {start, length}
  uint32_t seed;
  int64_t sample_begin;
  uint2* slab;
  int64_t slab_stride;
  int32_t* unit_n;            // [batch][n_units]
  int32_t* flags;
  uint32_t* ws_stat;
};

__global__ __launch_bounds__(64) void k_circular(CircularArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int sidx = (int)blockIdx.x;
  const int a = (int)(blockIdx.y + blockIdx.z * gridDim.y);
  if (a >= A.n_active) return;
  const UnitDev U = A.units_o[a];
  const int u = U.pad;
  const uint4 T = A.circ_unit[u];
  const uint2* __restrict__ iv = A.circ_iv + T.x;
  const uint2* __restrict__ W = A.ws + U.ws_off;
  const uint32_t* __restrict__ cdf = A.ws_cdf + U.ws_off;
  const int n = (int)T.y, nw = (int)T.z;
  const uint64_t wsum = T.w;
  uint2* out = A.slab + (int64_t)sidx * A.slab_stride + U.slab_off;
  const int cap = U.slab_cap;
  const uint32_t seed = unit_stream_seed(A.seed, A.sample_begin, sidx, A.n_units, u);

  WaveRng rng;
  rng.mt = lds;
  rng_seed(rng, seed, lane);
  rng_no_rows(rng); rng.seed = seed;

  int n_out = 0, status = 0;
  if (n > 0 && nw > 0 && wsum > 0) {
    const uint64_t r = rng_range(rng, T.w - 1u, lane);       // randint(0, Wsum): nothing drawn when Wsum is 1

    // piece index in the doubled W of linear position p (< 2 Wsum): the pieces ending at or before it
    auto piece_of = [&](uint64_t p) -> int {
      const bool second = p >= wsum;
      const uint32_t lp = (uint32_t)(second ? p - wsum : p);
      int lo = 0, hi = nw;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] < lp) lo = mid + 1; else hi = mid;      // (cumulated length <= lp)
      }
      return second ? nw + lo : lo;
    };
    auto start_of = [&](int g) -> uint64_t {                 // linear start of doubled piece g
      const int h = g >= nw ? g - nw : g;
      return (g >= nw ? wsum : 0ull) + (h ? (uint64_t)cdf[h - 1] + 1ull : 0ull);
    };

    // counting pass: pieces per interval, and those beyond the wrap
    uint32_t total = 0, wrapped = 0;
    for (int x0 = 0; x0 < n; x0 += kWave) {
      const int x = x0 + lane;
      uint32_t c = 0, w = 0;
      if (x < n) {
        const uint2 v = iv[x];
        const uint64_t q = r + v.x, e = q + v.y;
        const int g0 = piece_of(q), g1 = piece_of(e - 1);
        c = (uint32_t)(g1 - g0 + 1);
        w = g1 >= nw ? (uint32_t)(g1 - (g0 > nw ? g0 : nw) + 1) : 0u;
      }
      total += wave_total_u32(c);
      wrapped += wave_total_u32(w);
    }
    const uint32_t before_wrap = total - wrapped;
    if ((int)total > cap) {                                  // (cannot happen: cap >= n + |W| >= total)
      status |= kStatusOverflow;
    } else {
      // writing pass: walk index o + k -> rotated index (beyond the wrap: o + k - before_wrap, else o + k + wrapped)
      uint32_t carry_pieces = 0;
      for (int x0 = 0; x0 < n; x0 += kWave) {
        const int x = x0 + lane;
        uint64_t q = 0, e = 0;
        int g0 = 0;
        uint32_t c = 0;
        if (x < n) {
          const uint2 v = iv[x];
          q = r + v.x;
          e = q + v.y;
          g0 = piece_of(q);
          c = (uint32_t)(piece_of(e - 1) - g0 + 1);
        }
        const uint32_t cincl = wave_incl_sum_u32(c, lane);
        const uint32_t o = carry_pieces + cincl - c;
        for (uint32_t k = 0; k < c; ++k) {
          const int g = g0 + (int)k;
          const int h = g >= nw ? g - nw : g;
          const uint2 wp = W[h];
          const uint64_t gs = start_of(g), ge = gs + (wp.y - wp.x);
          const uint64_t ls = q > gs ? q : gs, le = e < ge ? e : ge;
          const uint32_t s = wp.x + (uint32_t)(ls - gs);
          const uint32_t walk = o + k;
          const uint32_t dst = g >= nw ? walk - before_wrap : walk + wrapped;
          if (dst < (uint32_t)cap) out[dst] = make_uint2(s, s + (uint32_t)(le - ls));
        }
        carry_pieces += (uint32_t)__builtin_amdgcn_readlane((int)cincl, kWave - 1);
      }
      n_out = (int)total;
    }
  }
  if (lane == 0) {
    A.unit_n[(int64_t)sidx * A.n_units + u] = status ? 0 : n_out;
    if (status) atomicOr(A.flags, status);
    *reinterpret_cast<uint4*>(A.ws_stat + ((int64_t)u * A.rec_stride + sidx) * 4) = make_uint4((uint32_t)n, rng.ndraws, 0u, 1u);
  }
}

}  // namespace gat
