// gat_universe.h -- SamplerUniverse on the device: k_universe, one wave per (sample, unit).  The reference has no such
// sampler; the contract is DESIGN.md section 5 ("k_universe") and tests/universe_model.py is the same in Python.
//
// The universe is the unit's workspace W: its m pieces are the candidates, and k of them share a base with a segment
// (problem creation, gat_prep_units.h: universe_hits).  A sample is k pieces of W chosen uniformly without replacement,
// every piece whole, in genome order.  Per work unit the stream is the per-unit one of every sampler here
// (numpy.random.seed((seed + sample*n_units + unit) mod 2^32)), run by the wave's in-LDS MT19937.
//
// The draw is Floyd's algorithm on the smaller side, c = min(k, m - k) marks in a table of m bits: for j = m - c .. m - 1,
// t = randint(0, j + 1); t is marked, or j when t is marked already (j is not: no earlier step could mark it).  Every step
// is one wave-uniform test-and-set in LDS, a chain of c dependent steps.  The marked pieces are the sample, or the unmarked
// ones when 2k > m (invert).  The write-out reads the table 64 words -- 2 048 pieces -- per wave step: a popcount per lane, a
// wave inclusive sum, a carry from step to step; every set bit h stores W[h] at its rank.  Exactly k pieces, the unit's
// slab capacity.
//
// LDS: the generator's state and the launch's mark table (UniverseArgs::table_words, from the largest active unit -- the
// waves a CU holds are what hides the chain, so no more than that), whole wave steps of 64 words.
#pragma once
#include "gat_kernels.h"

namespace gat {

static_assert(kUniverseFixedLdsBytes == kMtLdsWords * 4, "universe_max_pieces (gat_types.h) counts the generator's state");

struct UniverseArgs {
  const UnitDev* units_o;     // active units in launch order, unit id in `pad`
  int32_t n_units;
  int32_t n_active;
  int32_t rec_stride;         // ws_stat: [unit][rec_stride]
  const uint2* ws;            // W: the unit's workspace pieces at UnitDev::ws_off
  const uint4* univ_unit;     // per unit {k, m, c, invert}
  int32_t table_words;        // the mark table in LDS: a multiple of 64 words, >= ceil(m / 32) of every active unit
  uint32_t seed;
  int64_t sample_begin;
  uint2* slab;
  int64_t slab_stride;
  int32_t* unit_n;            // [batch][n_units]
  int32_t* flags;
  uint32_t* ws_stat;
};

__global__ __launch_bounds__(64) void k_universe(UniverseArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int sidx = (int)blockIdx.x;
  const int a = (int)(blockIdx.y + blockIdx.z * gridDim.y);
  if (a >= A.n_active) return;
  const UnitDev U = A.units_o[a];
  const int u = U.pad;
  const uint4 T = A.univ_unit[u];
  const uint2* __restrict__ W = A.ws + U.ws_off;
  const uint32_t k = T.x, m = T.y, c = T.z;
  const bool invert = T.w != 0u;
  uint2* out = A.slab + (int64_t)sidx * A.slab_stride + U.slab_off;
  const uint32_t cap = (uint32_t)U.slab_cap;
  const uint32_t seed = unit_stream_seed(A.seed, A.sample_begin, sidx, A.n_units, u);

  WaveRng rng;
  rng.mt = lds;
  rng_seed(rng, seed, lane);
  rng_no_rows(rng); rng.seed = seed;

  uint32_t* table = lds + kMtLdsWords;
  const uint32_t words = (m + 31u) >> 5;                       // of this unit
  const uint32_t steps = (words + (uint32_t)kWave - 1u) / (uint32_t)kWave;
  int n_out = 0, status = 0;
  if (k > cap || steps * (uint32_t)kWave > (uint32_t)A.table_words) {      // (cannot happen: cap >= k, the table is the launch's largest)
    status |= kStatusOverflow;
  } else if (k > 0) {
    for (uint32_t i = (uint32_t)lane; i < steps * (uint32_t)kWave; i += (uint32_t)kWave) table[i] = 0u;
    wave_sync();
    // the c marks: wave-uniform, every step reads the word the step before may have written
    for (uint32_t j = m - c; j < m; ++j) {
      const uint32_t t = rng_range(rng, j, lane);              // randint(0, j + 1)
      const uint32_t seen = rfl(table[t >> 5]) >> (t & 31u) & 1u;
      const uint32_t h = seen ? j : t;
      if (lane == 0) table[h >> 5] |= 1u << (h & 31u);
      wave_sync();
    }
    // write-out: the marked pieces, or the unmarked ones, at their rank
    uint32_t carry = 0;
    for (uint32_t s = 0; s < steps; ++s) {
      const uint32_t wi = s * (uint32_t)kWave + (uint32_t)lane;
      uint32_t bits = 0;
      if (wi < words) {
        bits = table[wi];
        if (invert) bits = ~bits;
        if (wi == words - 1u && (m & 31u)) bits &= (1u << (m & 31u)) - 1u;      // (the table's last word ends at piece m)
      }
      const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
      const uint32_t incl = wave_incl_sum_u32(cnt, lane);
      uint32_t o = carry + incl - cnt;
      while (bits) {
        const uint32_t h = wi * 32u + (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1u;
        if (o < cap && h < m) out[o] = W[h];
        ++o;
      }
      carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    }
    n_out = (int)carry;                                        // (== k)
  }
  if (lane == 0) {
    A.unit_n[(int64_t)sidx * A.n_units + u] = status ? 0 : n_out;
    if (status) atomicOr(A.flags, status);
    *reinterpret_cast<uint4*>(A.ws_stat + ((int64_t)u * A.rec_stride + sidx) * 4) = make_uint4(k, rng.ndraws, 0u, 1u);
  }
}

}  // namespace gat
