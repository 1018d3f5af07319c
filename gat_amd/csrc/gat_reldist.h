// gat_reldist.h -- where the segments of a list sit between the two points that flank them, as a fraction of the gap (the
// relative distance test: bedtools reldist, GenometriCorr), formed where the lists are (gat_list_reldist,
// gat_sample_reldist_enrichment).  gat_reldist_bins.h has the conventions: a segment stands for its midpoint m, it is inside
// iff two points of the (track, group) flank it, p_{j-1} <= m < p_j, and then falls into one of B bins over [0, 0.5].  For a
// list L over the groups g and a point track t, W = B + 3 values:
//
//   v_b = the inside segments of bin b      area = floor(D 10^6 / (n B^2)), D = sum_b |B C_b - (b + 1) n|      n = inside      outside
//
// and over the samples of a range, per (track, value), the five words of gat_null_words.h against the caller's obs.  The
// (samples x tracks x values) matrix is never formed.  The lists need be neither sorted nor disjoint: a segment counts on its
// own, whatever lies beside it.
//
// The layout is k_profile's (gat_profile.h).  A workgroup (256 threads, 4 waves) owns one point TRACK and a run of lists.  It
// stages, per group, what the search starts in: the positions of the (track, group) -- all of them when there are at most L,
// else the last position of each block of `stride` (block_table / block_search, gat_lists.h), the search ending in global
// memory; L == 0: the search runs in global memory -- and, when it folds, the track's obs row.
//
// A WAVE takes one list at a time, over ALL groups (the values sum over them), and owns a private histogram of B 32-bit words
// in LDS; inside and outside are counted in registers.  The lanes stride over the segments of (list, g): one search for the
// first point >= m + 1, two position reads, one LDS atomic (two lanes may meet in a bin).  When the list is through, the wave
// sweeps the bins 64 at a time -- consecutive lanes, consecutive words, a carry from round to round, as k_profile sweeps its
// difference array; a lane that owned 16 consecutive bins at B = 1024 would read LDS at a stride of 16 words -- and every round
// is one inclusive scan: n is known from the registers before the sweep, so C_b and the term of D are formed in the round
// that reads v_b.  The wave clears the words behind it and either STORES the values (one owner per (list, track, value): a
// plain store into an output the caller zeroed) or FOLDS them into the workgroup's per-value accumulators in LDS -- for v > 0
// only.  At the end the workgroup adds the values with n_pos > 0 to the result: consecutive lanes, consecutive values.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_reldist_bins.h"
#include "gat_null_words.h"

namespace gat {

struct ReldistArgs {
  ListSet lists;              // n_lists x n_groups of them
  int32_t n_lists;
  int32_t n_groups;
  int32_t n_tracks;
  int32_t lists_per_block;
  int32_t bins;               // B
  int32_t lds_points;         // L: the dynamic LDS is reldist_lds_bytes(B, L, n_groups, STORE)
  const uint32_t* pos;        // the points' positions, strictly ascending per (track, group)
  const int64_t* point_off;   // [n_tracks * n_groups + 1], track-major, from 0
  const long long* obs;       // FOLD: [n_tracks][W]
  unsigned long long* out;    // STORE: [n_lists][n_tracks][W]; FOLD: [n_tracks][W][kNullWords]
};

// first k in [0, K) with pos[k] >= x, K: none -- from the staged level (bt: its block_table) where there is one
__device__ __forceinline__ int reldist_first_point(const uint32_t* level, int L, const BlockTable& bt, const uint32_t* __restrict__ pos, int K, uint32_t x) {
  if (L > 0) return block_search<false>(level, bt.nl, K, bt.stride, x, [&](int m) { return pos[m]; });
  int lo = 0, hi = K;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (pos[m] >= x) hi = m; else lo = m + 1;
  }
  return lo;
}

template <bool STORE>
__global__ __launch_bounds__(kReldistThreads) void k_reldist(ReldistArgs A) {
  extern __shared__ unsigned long long reldist_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int B = A.bins, W = B + kReldistExtra, L = A.lds_points, G = A.n_groups;
  const int track = (int)blockIdx.x;
  unsigned long long* l_sum = reldist_lds;
  unsigned long long* l_sumsq = l_sum + (STORE ? 0 : W);
  unsigned long long* l_obs = l_sumsq + (STORE ? 0 : W);
  uint32_t* l_pos = reinterpret_cast<uint32_t*>(l_obs + (STORE ? 0 : W));
  uint32_t* l_less = l_pos + (STORE ? 0 : W);
  uint32_t* l_eq = l_less + (STORE ? 0 : W);
  uint32_t* hists = l_eq + (STORE ? 0 : W);
  uint32_t* hist = hists + (size_t)wave * B;
  uint32_t* tab = hists + (size_t)kReldistWaves * B;          // [group][level]

  const int64_t* __restrict__ off = A.point_off + (int64_t)track * G;
  {                           // everything up to the staged positions starts at 0
    uint32_t* words = reinterpret_cast<uint32_t*>(reldist_lds);
    const int n_words = (int)(tab - words);
    for (int k = tid; k < n_words; k += kReldistThreads) words[k] = 0u;
  }
  for (int64_t k = tid; k < (int64_t)G * L; k += kReldistThreads) {
    const int lv = (int)(k % L), g = (int)(k / L);
    const int64_t b = off[g];
    const int K = (int)(off[g + 1] - b);
    const BlockTable bt = block_table(K, L);
    tab[k] = lv < bt.nl ? A.pos[b + min(K - 1, (lv + 1) * bt.stride - 1)] : 0u;
  }
  __syncthreads();
  if constexpr (!STORE) {
    for (int c = tid; c < W; c += kReldistThreads) l_obs[c] = (unsigned long long)A.obs[(int64_t)track * W + c];
    __syncthreads();
  }

  // value c of list i: stored, or folded into the workgroup's words of the cell (v > 0)
  auto emit = [&](int i, int c, unsigned long long v) {
    if constexpr (STORE) {
      A.out[((int64_t)i * A.n_tracks + track) * W + c] = v;
    } else {
      null_words_count(v, l_obs[c], [&](NullWord x, unsigned long long y) {
        if (x == kNullSum) atomicAdd(&l_sum[c], y);
        else if (x == kNullSumsq) atomicAdd(&l_sumsq[c], y);
        else atomicAdd(&(x == kNullPos ? l_pos : x == kNullLess ? l_less : l_eq)[c], (uint32_t)y);
      });
    }
  };

  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  for (int i = i0 + wave; i < i1; i += kReldistWaves) {
    uint32_t in = 0u, outside = 0u;                     // this lane's segments
    for (int g = 0; g < G; ++g) {
      const int64_t a0 = off[g];                        // (uniform)
      const int K = (int)(off[g + 1] - a0);
      int n;
      const uint2* __restrict__ seg = list_at(A.lists, i, g, G, n);
      const uint32_t* __restrict__ P = A.pos + a0;
      const uint32_t* level = tab + (int64_t)g * L;
      const BlockTable bt = block_table(K, max(L, 1));
      for (int j = lane; j < n; j += kWave) {
        const uint2 sg = seg[j];
        if (sg.y <= sg.x) continue;
        const uint32_t m = reldist_midpoint(sg.x, sg.y);
        const int k = K < 2 ? 0 : reldist_first_point(level, L, bt, P, K, m + 1u);
        if (k == 0 || k == K) { outside += 1u; continue; }
        atomicAdd(&hist[reldist_bin(m, P[k - 1], P[k], B)], 1u);
        in += 1u;
      }
    }
    const uint32_t n_in = wave_sum_u32(in), n_out = wave_sum_u32(outside);
    if (n_in == 0u && n_out == 0u) continue;            // no segment in this list
    unsigned long long D = 0ull;
    if (n_in > 0u) {
      wave_fence();
      uint32_t carry = 0u;
      for (int base = 0; base < B; base += kWave) {
        const int b = base + lane;
        const uint32_t v = b < B ? hist[b] : 0u;
        const uint32_t C = carry + wave_incl_sum_u32(v, lane);
        carry = (uint32_t)__builtin_amdgcn_readlane((int)C, kWave - 1);
        if (b < B) D += reldist_area_term(C, n_in, b, B);
        if (v == 0u) continue;
        hist[b] = 0u;
        emit(i, b, v);
      }
      D = (unsigned long long)wave_sum_i64((long long)D);
      wave_fence();
    }
    const unsigned long long extra = lane == 0 ? reldist_area(D, n_in, B) : lane == 1 ? n_in : lane == 2 ? n_out : 0ull;
    if (lane < kReldistExtra && extra > 0ull) emit(i, B + lane, extra);
  }

  if constexpr (!STORE) {
    __syncthreads();
    for (int c = tid; c < W; c += kReldistThreads) {
      const uint32_t np = l_pos[c];
      if (np == 0u) continue;
      null_words_flush(A.out + ((int64_t)track * W + c) * kNullWords, np, l_sum[c], l_sumsq[c], l_less[c], l_eq[c]);
    }
  }
}

}  // namespace gat
