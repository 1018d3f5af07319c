// gat_local_permute.h -- SamplerLocalPermutation (gat/Engine.pyx:1117-1229) on the device: k_permute_local, one wave per
// (sample, unit).
//
// Per work unit the stream is random.seed((seed + sample*n_units + unit) mod 2^32), CPython's seeding and _randbelow on the
// wave's in-LDS MT19937, as in k_permute.  The reference walks the unit's workspace pieces in order and draws, for every
// piece with working segments, random.shuffle(lengths), n x randint(0, free) (the points, sorted) and one more (the shift)
// from that ONE stream: where a piece's draws begin depends on the rejections of the pieces before it, so the pieces are
// serial within the wave.  Problem creation (gat_prep_units.h: local_permute_tables) laid down, per active piece, {first, n,
// work_end, free}: the working segments are the run [first, first + n) of the unit's list (getOverlappingSegments' set: the
// segment in front of the piece is in it whether it reaches the piece or not) and work_start is 0 -- the reference's
// min() / max() of that set return 0 (their assertions fire where nothing can be raised), so every piece is permuted over
// [0, work_end) and free = work_end - sum(lengths).
//
// The reference's walk has a closed form (tests/local_permutation_model.py is the walk itself): with S = work_end, segment
// x of the shuffled list covers [q_x, q_x + L_x) modulo S, q_x = shift + points[x] + the lengths before it; q_x + L_x <=
// S + free < 2S, so the walk wraps at most once: q >= S gives (q - S, e - S), e < S gives (q, e), else (q, S) and
// (0, e - S) -- either may be empty.  A segment gives at most two pieces, a piece of n working segments at most 2n, and the
// sum of 2n is the capacity of the unit's slab region.  The reference assigns start and end to C ints: the first
// segment that reaches S raises OverflowError when its unwrapped start (q > S) or end is beyond 2^31 - 1 --
// kStatusCoordRange.  After the last piece the list is sorted and merged with SegmentList.normalize's rule (overlaps
// united, adjacent pieces kept apart, empties dropped), which the reference applies after every piece to the same effect:
// in LDS when it fits the launch's list_cap, in the slab otherwise.
//
// The draw chain.  A piece with one working segment draws two _randbelow(free + 1) and nothing else, one with two draws
// _randbelow(2) and three _randbelow(free + 1); the bounds are in the tables, only the rejections are dynamic.  A run of
// consecutive pieces of one or two working segments (up to 64 draws) is resolved together (local_permute_small_batch): the
// draws' bounds are laid out in LDS in stream order, lane i of the block of raw words tests word i against the bound of the
// draw it would serve if no word before it were rejected, a ballot finds the first rejection, the draws before it are final
// and the lanes behind it move up by one word and test again -- a ballot and an LDS read per rejection instead of a
// block reload, ballot and read-lane per draw.  Larger pieces go one at a time (local_permute_piece, py_randbelow_batch for
// the points).  `simple` (context option GAT_LPERM_SIMPLE) sends every piece down that path: the A/B of
// profiles/r08_local_permutation.txt.  `no_normalize` (GAT_EXP_LPERM_NO_NORMALIZE) is a timing experiment with wrong
// results: the final sort and merge are skipped and the units' lists are left empty -- the draw chain alone.
//
// Empty pieces are not stored: the pieces of a step are compacted with a ballot and a prefix count.
//
// A piece's lengths and points live in LDS when n <= lds_cap, else at the top of the unit's slab region (which then has 2n
// entries beyond the pieces' slots).
#pragma once
#include "gat_kernels.h"

namespace gat {

struct LocalPermuteArgs {
  const UnitDev* units_o;     // active units in launch order, unit id in `pad`
  int32_t n_units;
  int32_t n_active;
  int32_t rec_stride;         // ws_stat: [unit][rec_stride]
  int32_t lds_cap;            // working segments of ONE piece the LDS buffers hold
  int32_t list_cap;           // pieces of the final list the same LDS holds for the sort and merge
  int32_t simple;             // every piece on its own (no batched small-piece path)
  int32_t no_normalize;       // timing experiment: no final sort and merge, empty lists
  const uint4* lp_unit;       // per unit {pieces offset, active pieces, lengths offset, sum of n}
  const uint4* lp_piece;      // per active piece {first, n, work_end, free}
  const uint32_t* lp_len;     // the units' segment lengths, list order
  uint32_t seed;
  int64_t sample_begin;
  uint2* slab;
  int64_t slab_stride;
  int32_t* unit_n;            // [batch][n_units]
  int32_t* flags;
  uint32_t* ws_stat;
};

constexpr int kLpBatchDraws = 64;      // draws a small-piece batch resolves together (bnd / vals in LDS)

// the pieces segment [q, e) of the walk over [0, S) gives, empties dropped: put(start, end) is called for each
template <typename Put>
__device__ __forceinline__ void local_permute_pieces_of(uint64_t q, uint64_t e, uint32_t S, Put put) {
  if (q >= S) { if (e != q) put((uint32_t)(q - S), (uint32_t)(e - S)); }
  else if (e < S) { if (e != q) put((uint32_t)q, (uint32_t)e); }
  else {
    if (q != S) put((uint32_t)q, S);
    if (e != S) put(0u, (uint32_t)(e - S));
  }
}

// A run of np consecutive pieces of one or two working segments, piece i in lane i (P: its record), D <= kLpBatchDraws draws
// in all.  Returns the pieces written at dst.
__device__ __forceinline__ int local_permute_small_batch(WaveRng& rng, const uint4 P, int np, const uint32_t* __restrict__ len_all,
                                                         uint32_t* bnd, uint32_t* vals, uint2* dst, int lane, int& status) {
  const bool mine = lane < np;
  const int n = mine ? (int)P.y : 0;
  const uint32_t incl = wave_incl_sum_u32((uint32_t)(2 * n), lane);
  const int off = (int)incl - 2 * n;
  const int D = __builtin_amdgcn_readlane((int)incl, kWave - 1);
  if (mine) {                                             // the draws' bounds in stream order
    const uint32_t b = P.w + 1u;
    if (n == 2) { bnd[off] = 2u; bnd[off + 1] = b; bnd[off + 2] = b; bnd[off + 3] = b; }
    else { bnd[off] = b; bnd[off + 1] = b; }
  }
  wave_sync();
  int d0 = 0;                                             // draws resolved
  while (d0 < D) {
    py_window(rng, lane);
    const int base = rng.pos & ~(kWave - 1), offw = rng.pos - base, lim = kMtN - base < kWave ? kMtN - base : kWave;
    int w0 = offw;                                        // the block's first unused word
    while (d0 < D && w0 < lim) {
      const int d = d0 + lane - w0;                       // the draw word `lane` serves if none before it is rejected
      const bool act = lane >= w0 && lane < lim && d < D;
      const uint32_t b = act ? bnd[d] : 1u;
      const uint32_t v = rng.rbuf >> (uint32_t)__builtin_clz(b);
      const uint64_t am = __ballot(act), rej = __ballot(act && v >= b);
      const int stop = rej ? (int)__builtin_ctzll(rej) : w0 + __popcll(am);
      if (act && lane < stop) vals[d] = v;
      d0 += stop - w0;
      w0 = rej ? stop + 1 : stop;
    }
    rng.ndraws += (uint32_t)(w0 - offw);
    rng.pos = base + w0;
  }
  wave_sync();
  // the walk of every piece in closed form; counted, then written behind the lanes before
  uint64_t q0 = 0, e0 = 0, q1 = 0, e1 = 0;
  uint32_t S = 0;
  bool bad = false;
  if (mine) {
    S = P.z;
    uint32_t L0 = len_all[P.x];
    if (n == 2) {
      uint32_t L1 = len_all[P.x + 1u];
      if (vals[off] == 0u) { const uint32_t t = L0; L0 = L1; L1 = t; }        // shuffle: j = _randbelow(2), x[1] <-> x[j]
      const uint32_t a = vals[off + 1], c = vals[off + 2], sh = vals[off + 3];
      q0 = (uint64_t)sh + (a < c ? a : c); e0 = q0 + L0;
      q1 = (uint64_t)sh + (a < c ? c : a) + L0; e1 = q1 + L1;
    } else {
      q0 = (uint64_t)vals[off] + vals[off + 1]; e0 = q0 + L0;
      q1 = e1 = 0;
    }
    // the first segment to reach S: its unwrapped start or end beyond 2^31 - 1 is the reference's OverflowError
    if (e0 >= S) bad = (q0 > S ? q0 : e0) > 0x7fffffffull;
    else if (n == 2 && e1 >= S) bad = (q1 > S ? q1 : e1) > 0x7fffffffull;
  }
  if (__ballot(bad)) status |= kStatusCoordRange;
  uint32_t c = 0;
  if (mine) {
    local_permute_pieces_of(q0, e0, S, [&](uint32_t, uint32_t) { ++c; });
    if (n == 2) local_permute_pieces_of(q1, e1, S, [&](uint32_t, uint32_t) { ++c; });
  }
  const uint32_t cincl = wave_incl_sum_u32(c, lane);
  if (mine) {
    uint2* w = dst + (cincl - c);
    local_permute_pieces_of(q0, e0, S, [&](uint32_t a, uint32_t b) { *w++ = make_uint2(a, b); });
    if (n == 2) local_permute_pieces_of(q1, e1, S, [&](uint32_t a, uint32_t b) { *w++ = make_uint2(a, b); });
  }
  return __builtin_amdgcn_readlane((int)cincl, kWave - 1);
}

// one piece: the draws, and its pieces (at most 2n) at dst; returns how many
template <bool MEM>
__device__ __forceinline__ int local_permute_piece(WaveRng& rng, const uint32_t* __restrict__ len_src, uint32_t* lenb, uint2* ptb,
                                                    uint2* dst, int n, uint32_t S, uint32_t free_len, int lane, int& status) {
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

  uint32_t carry_len = 0;
  int written = 0;
  bool reached = false;                                   // some segment before this chunk reached S: the walk has wrapped
  for (int x0 = 0; x0 < n; x0 += kWave) {
    const int x = x0 + lane;
    const bool valid = x < n;
    const uint32_t pt = valid ? ptb[x].x : 0u, L = valid ? lenb[x] : 0u;
    const uint32_t incl = wave_incl_sum_u32(L, lane);
    const uint64_t q = shift + pt + carry_len + (incl - L), e = q + L;
    const uint64_t m = __ballot(valid && e >= S);
    if (!reached && m) {
      const int f = (int)__builtin_ctzll(m);
      if (__ballot(lane == f && (q > S ? q : e) > 0x7fffffffull)) status |= kStatusCoordRange;
      reached = true;
    }
    uint32_t c = 0;
    if (valid) local_permute_pieces_of(q, e, S, [&](uint32_t, uint32_t) { ++c; });
    const uint32_t cincl = wave_incl_sum_u32(c, lane);
    if (valid) {
      uint2* w = dst + written + (cincl - c);
      local_permute_pieces_of(q, e, S, [&](uint32_t a, uint32_t b) { *w++ = make_uint2(a, b); });
    }
    written += __builtin_amdgcn_readlane((int)cincl, kWave - 1);
    carry_len += (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
  }
  return written;
}

__global__ __launch_bounds__(64) void k_permute_local(LocalPermuteArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int sidx = (int)blockIdx.x;
  const int a = (int)(blockIdx.y + blockIdx.z * gridDim.y);
  if (a >= A.n_active) return;
  const UnitDev U = A.units_o[a];
  const int u = U.pad;
  const uint4 T = A.lp_unit[u];
  const uint4* __restrict__ pieces = A.lp_piece + T.x;
  const uint32_t* __restrict__ len_all = A.lp_len + T.z;
  const int n_pieces = (int)T.y;
  uint2* out = A.slab + (int64_t)sidx * A.slab_stride + U.slab_off;
  const int cap = U.slab_cap;
  const uint32_t seed = unit_stream_seed(A.seed, A.sample_begin, sidx, A.n_units, u);

  WaveRng rng;
  rng.mt = lds;
  rng_no_rows(rng); rng.seed = seed;
  rng_seed_by_array(rng, seed, lane);

  const int cap_even = (A.lds_cap + 1) & ~1;
  uint32_t* bnd = lds + kMtLdsWords;
  uint32_t* vals = bnd + kLpBatchDraws;
  uint32_t* work = vals + kLpBatchDraws;                  // a piece's lengths and points; the final list
  uint32_t* lenb_lds = work;
  uint2* ptb_lds = reinterpret_cast<uint2*>(work + cap_even);

  int nout = 0, status = 0;
  int k = 0;
  while (k < n_pieces && !status) {
    if (!A.simple) {
      // the run of pieces of one or two working segments from k on, as far as kLpBatchDraws draws go
      const uint4 Q = k + lane < n_pieces ? pieces[k + lane] : make_uint4(0u, 3u, 0u, 0u);
      const uint64_t big = __ballot(Q.y > 2u);
      const int run = big ? (int)__builtin_ctzll(big) : kWave;
      const uint32_t dincl = wave_incl_sum_u32(lane < run ? 2u * Q.y : 0u, lane);
      const int np = __popcll(__ballot(lane < run && dincl <= (uint32_t)kLpBatchDraws));
      if (np >= 2) {
        const uint32_t slots = (uint32_t)__builtin_amdgcn_readlane((int)dincl, np - 1);     // 2n over the run
        if (nout + (int)slots > cap) { status |= kStatusOverflow; break; }                  // (cannot happen: cap >= the sum of 2n)
        nout += local_permute_small_batch(rng, Q, np, len_all, bnd, vals, out + nout, lane, status);
        k += np;
        continue;
      }
    }
    const uint4 P = pieces[k];
    const int n = (int)P.y;
    if (nout + 2 * n > cap) { status |= kStatusOverflow; break; }     // (cannot happen: cap >= the sum of 2n)
    if (n <= A.lds_cap) {
      nout += local_permute_piece<false>(rng, len_all + P.x, lenb_lds, ptb_lds, out + nout, n, P.z, P.w, lane, status);
    } else if (nout + 4 * n <= cap) {
      // (the lengths and points at the top of the region, beyond every piece's slots)
      uint2* ptb = out + (cap - n);
      uint32_t* lenb = reinterpret_cast<uint32_t*>(out + (cap - 2 * n));
      nout += local_permute_piece<true>(rng, len_all + P.x, lenb, ptb, out + nout, n, P.z, P.w, lane, status);
    } else {
      status |= kStatusOverflow;
    }
    ++k;
  }

  // sample.normalize(): sort by start, unite overlaps, keep adjacent pieces apart, drop empties
  int n = status || A.no_normalize ? 0 : nout;
  __syncthreads();                                        // (the stores to the slab, seen by the wave)
  if (n > 1) {
    if (n <= A.list_cap) {
      uint2* seg = reinterpret_cast<uint2*>(work);
      for (int j = lane; j < n; j += kWave) seg[j] = out[j];
      wave_sort_auto(seg, n, lane);
      n = wave_merge0<false, true>(seg, n, lane);
      for (int j = lane; j < n; j += kWave) out[j] = seg[j];
    } else {
      wave_sort_by_start<true>(out, n, lane);
      n = wave_merge0<true, true>(out, n, lane);
    }
  }
  if (lane == 0) {
    A.unit_n[(int64_t)sidx * A.n_units + u] = n;
    if (status) atomicOr(A.flags, status);
    *reinterpret_cast<uint4*>(A.ws_stat + ((int64_t)u * A.rec_stride + sidx) * 4) = make_uint4(T.w, rng.ndraws, 0u, 1u);
  }
}

}  // namespace gat
