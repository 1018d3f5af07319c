// gat_permute.h -- SamplerGlobalPermutation (gat/Engine.pyx:1234-1386) on the device: k_permute, one wave per (sample, unit).
//
// Per work unit the stream is random.seed((seed + sample*n_units + unit) mod 2^32) -- the per-unit family of every sampler
// here with CPython's seeding (rng_seed_by_array) and _randbelow (py_randbelow*) on the wave's in-LDS MT19937.
// Problem creation (gat_prep_units.h: permute_tables) laid down, per unit, the working segments' lengths in list order and W,
// the workspace extended by them and merge(0)ed, with its cumulated lengths and free = Wsum - sum(lengths).
//
// The draws, in the reference's order: random.shuffle(lengths) (j = _randbelow(i + 1) for i = n-1..1, then the swap --
// the one serial chain, in LDS), n x randint(0, free) (the points, sorted) and one more (shift).  The reference's walk
// then has a closed form (tests/permutation_model.py): segment x covers the linear range [q_x, q_x + L_x) of W modulo
// Wsum, q_x = shift + points[x] + P_x, P_x the lengths before it; the ranges never overlap and the walk spans less than
// Wsum from shift, so normalize() only rotates the list to its lowest coordinate -- the pieces at linear positions >= Wsum
// come first.  A counting pass gives the pieces per segment and how many lie beyond the wrap; the writing pass puts every
// piece at its rotated place.  At most n + |W| pieces.
//
// The lengths and points live in LDS when the unit fits the launch's lds_cap, else at the top of the unit's slab region
// (its capacity is 2n + |W|: the pieces, at most n + |W|, are written below the points, which are read as they go).
#pragma once
#include "gat_kernels.h"

namespace gat {

struct PermuteArgs {
  const UnitDev* units_o;     // active units in launch order, unit id in `pad`
  int32_t n_units;
  int32_t n_active;
  int32_t rec_stride;         // ws_stat: [unit][rec_stride]
  int32_t lds_cap;            // working segments the LDS buffers hold
  const uint4* perm_unit;     // per unit {lengths offset, W offset, |W|, free}
  const uint32_t* perm_len;   // the working segments' lengths, list order
  const uint2* perm_w;        // W's pieces
  const uint32_t* perm_cum;   // W's cumulated lengths: entry j = bases of pieces 0..j
  uint32_t seed;
  int64_t sample_begin;
  uint2* slab;
  int64_t slab_stride;
  int32_t* unit_n;            // [batch][n_units]
  int32_t* flags;
  uint32_t* ws_stat;
};

template <bool MEM>
__device__ __forceinline__ void permute_unit(const PermuteArgs& A, WaveRng& rng, uint32_t* lenb, uint2* ptb, uint2* out,
                                             int cap, int n, const uint4 T, int lane, int& n_out, int& status) {
  const uint32_t* __restrict__ len_src = A.perm_len + T.x;
  const uint2* __restrict__ W = A.perm_w + T.y;
  const uint32_t* __restrict__ cum = A.perm_cum + T.y;
  const int nw = (int)T.z;
  const uint32_t free_len = T.w;
  const uint64_t wsum = cum[nw - 1];

  for (int j = lane; j < n; j += kWave) lenb[j] = len_src[j];
  wave_sync<MEM>();
  // random.shuffle(lengths): lane 0 swaps while the wave draws the next index
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)py_randbelow(rng, (uint32_t)(i + 1), lane);
    if (lane == 0) {
      const uint32_t a = lenb[i], b = lenb[j];
      lenb[i] = b;
      lenb[j] = a;
    }
  }
  // n x randint(0, free), sorted; then shift = randint(0, free)
  py_randbelow_batch(rng, free_len + 1u, n, lane, [&](int i, uint32_t v) { ptb[i] = make_uint2(v, 0u); });
  const uint64_t shift = py_randbelow(rng, free_len + 1u, lane);
  wave_sync<MEM>();
  wave_sort_auto<MEM>(ptb, n, lane);
  wave_sync<MEM>();
  for (int j = lane; j < n; j += kWave) ptb[j].y = lenb[j];       // (the lengths' buffer is free from here on)
  wave_sync<MEM>();

  // piece index in the doubled W of linear position p (< 2 Wsum): the pieces ending at or before it
  auto piece_of = [&](uint64_t p) -> int {
    const bool second = p >= wsum;
    const uint32_t lp = (uint32_t)(second ? p - wsum : p);
    int lo = 0, hi = nw;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] <= lp) lo = mid + 1; else hi = mid;
    }
    return second ? nw + lo : lo;
  };
  auto start_of = [&](int g) -> uint64_t {                  // linear start of doubled piece g
    const int h = g >= nw ? g - nw : g;
    return (g >= nw ? wsum : 0ull) + (h ? (uint64_t)cum[h - 1] : 0ull);
  };

  // counting pass: pieces per segment, and those beyond the wrap
  uint32_t carry_len = 0, total = 0, wrapped = 0;
  for (int x0 = 0; x0 < n; x0 += kWave) {
    const int x = x0 + lane;
    const uint2 pl = x < n ? ptb[x] : make_uint2(0u, 0u);
    const uint32_t incl = wave_incl_sum_u32(pl.y, lane);
    uint32_t c = 0, w = 0;
    if (x < n) {
      const uint64_t q = shift + pl.x + carry_len + incl - pl.y, e = q + pl.y;
      const int g0 = piece_of(q), g1 = piece_of(e - 1);
      c = (uint32_t)(g1 - g0 + 1);
      w = g1 >= nw ? (uint32_t)(g1 - (g0 > nw ? g0 : nw) + 1) : 0u;
    }
    carry_len += (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    total += wave_total_u32(c);
    wrapped += wave_total_u32(w);
  }
  const uint32_t before_wrap = total - wrapped;
  if ((int)total > cap) { status |= kStatusOverflow; n_out = 0; return; }   // (cannot happen: cap >= n + |W| >= total)

  // writing pass: walk index o + k -> rotated index (beyond the wrap: o + k - before_wrap, else o + k + wrapped)
  carry_len = 0;
  uint32_t carry_pieces = 0;
  for (int x0 = 0; x0 < n; x0 += kWave) {
    const int x = x0 + lane;
    const uint2 pl = x < n ? ptb[x] : make_uint2(0u, 0u);
    const uint32_t incl = wave_incl_sum_u32(pl.y, lane);
    uint64_t q = 0, e = 0;
    int g0 = 0;
    uint32_t c = 0;
    if (x < n) {
      q = shift + pl.x + carry_len + incl - pl.y;
      e = q + pl.y;
      g0 = piece_of(q);
      c = (uint32_t)(piece_of(e - 1) - g0 + 1);
    }
    const uint32_t cincl = wave_incl_sum_u32(c, lane);
    const uint32_t o = carry_pieces + cincl - c;
    for (uint32_t k = 0; k < c; ++k) {
      const int g = g0 + (int)k;
      const int h = g >= nw ? g - nw : g;
      const uint64_t gs = start_of(g), ge = gs + (W[h].y - W[h].x);
      const uint64_t ls = q > gs ? q : gs, le = e < ge ? e : ge;
      const uint32_t s = W[h].x + (uint32_t)(ls - gs);
      const uint32_t walk = o + k;
      const uint32_t dst = g >= nw ? walk - before_wrap : walk + wrapped;
      if (dst < (uint32_t)cap) out[dst] = make_uint2(s, s + (uint32_t)(le - ls));
    }
    carry_len += (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    carry_pieces += (uint32_t)__builtin_amdgcn_readlane((int)cincl, kWave - 1);
  }
  n_out = (int)total;
}

__global__ __launch_bounds__(64) void k_permute(PermuteArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int sidx = (int)blockIdx.x;
  const int a = (int)(blockIdx.y + blockIdx.z * gridDim.y);
  if (a >= A.n_active) return;
  const UnitDev U = A.units_o[a];
  const int u = U.pad;
  const uint4 T = A.perm_unit[u];
  uint2* out = A.slab + (int64_t)sidx * A.slab_stride + U.slab_off;
  const int cap = U.slab_cap;
  const int n = (int)U.hist_total;
  const uint32_t seed = unit_stream_seed(A.seed, A.sample_begin, sidx, A.n_units, u);

  WaveRng rng;
  rng.mt = lds;
  rng_no_rows(rng); rng.seed = seed;
  rng_seed_by_array(rng, seed, lane);

  int n_out = 0, status = 0;
  if (n > 0 && T.z > 0) {
    if (n <= A.lds_cap) {
      const int cap_even = (A.lds_cap + 1) & ~1;
      uint32_t* lenb = lds + kMtLdsWords;
      uint2* ptb = reinterpret_cast<uint2*>(lds + kMtLdsWords + cap_even);
      permute_unit<false>(A, rng, lenb, ptb, out, cap, n, T, lane, n_out, status);
    } else if (cap >= 2 * n + (int)T.z) {
      uint2* ptb = out + (cap - n);
      uint32_t* lenb = reinterpret_cast<uint32_t*>(out + (cap - 2 * n));
      permute_unit<true>(A, rng, lenb, ptb, out, cap, n, T, lane, n_out, status);
    } else {
      status |= kStatusOverflow;
    }
  }
  __syncthreads();
  if (lane == 0) {
    A.unit_n[(int64_t)sidx * A.n_units + u] = status ? 0 : n_out;
    if (status) atomicOr(A.flags, status);
    *reinterpret_cast<uint4*>(A.ws_stat + ((int64_t)u * A.rec_stride + sidx) * 4) = make_uint4((uint32_t)n, rng.ndraws, 0u, 1u);
  }
}

}  // namespace gat
