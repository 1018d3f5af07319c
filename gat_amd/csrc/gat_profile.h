// gat_profile.h -- how the segments of a list are distributed around a class of points (transcription start sites, motif
// centres, exon ends), formed where the lists are (gat_list_profile, gat_sample_profile_enrichment).  An anchor is (a, sigma);
// with w = bin_size, H = half_bins, R = H * w and B = 2 H offset bins (gat_profile_bins.h has the conventions), for a
// normalized list L over the groups g and an anchor track t
//
//   v(L, t, b) = sum over g, over (a, sigma) in A_{t,g}, over q in L_g of  #{ x in q : bin(x; a, sigma) = b }      0 <= v <= K_t * w
//
// (GAT_PROFILE_MIDPOINTS: q replaced by its midpoint base), a base counting once per anchor whose window holds it; and over the
// samples of a range, per (track, bin), the five words of gat_null_words.h against the caller's obs.  The (samples x tracks x
// bins) matrix is never formed.
//
// A workgroup (256 threads, 4 waves) owns one anchor TRACK and a run of lists.  It stages, per group, what the search for the
// first anchor of a segment starts in: the positions of the (track, group) -- all of them when there are at most L, else the
// last position of each block of `stride` (block_table / block_search, gat_lists.h), the search ending in global memory; L == 0:
// the search runs in global memory -- and, when it folds, the track's obs row.
//
// A WAVE takes one list at a time, over ALL groups (v sums over them: nothing is classified before the last), and owns a private
// vector in LDS: per bin a 32-bit sum of the pieces that cover the bin in part and a 32-bit difference array of "covered
// whole", as k_local has it -- a piece over many bins costs four adds.  The list is disjoint, so one anchor sends at most w
// bases into a bin: a bin is covered whole at most once per anchor, and no word passes K_t * w < 2^32 (the host refuses
// more).  The lanes stride over the segments of (list, g); a lane searches once for the first anchor at or beyond s - R, walks
// the anchors below e + R, clips each pair exactly by strand (profile_piece) and adds with LDS atomics (two lanes may meet in a
// bin).  When the list is through, the wave sweeps the touched range, scans the difference array, forms v, clears the words
// behind it, and either STORES v (one owner per (list, track, bin): a plain store into an output the caller zeroed) or FOLDS
// it into the workgroup's per-bin accumulators in LDS -- for v > 0 only.  At the end the workgroup adds the bins with
// n_pos > 0 to the result: consecutive lanes, consecutive bins.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_profile_bins.h"
#include "gat_null_words.h"

namespace gat {

struct ProfileArgs {
  ListSet lists;              // n_lists x n_groups of them, every one normalized
  int32_t n_lists;
  int32_t n_groups;
  int32_t n_tracks;
  int32_t lists_per_block;
  int32_t bins;               // B = 2 * half_bins
  int32_t lds_anchors;        // L: the dynamic LDS is profile_lds_bytes(B, L, n_groups, STORE)
  int32_t midpoints;          // GAT_PROFILE_MIDPOINTS
  int64_t bin_size;           // w
  int64_t reach;              // R
  const uint32_t* pos;        // the anchors' positions and strands (1: minus), ascending per (track, group)
  const uint8_t* minus;
  const int64_t* anchor_off;  // [n_tracks * n_groups + 1], track-major, from 0
  const long long* obs;       // FOLD: [n_tracks][B]
  unsigned long long* out;    // STORE: [n_lists][n_tracks][B]; FOLD: [n_tracks][B][kNullWords]
};

// first k in [0, K) with pos[k] >= x, K: none -- from the staged level (bt: its block_table) where there is one
__device__ __forceinline__ int profile_first_anchor(const uint32_t* level, int L, const BlockTable& bt, const uint32_t* __restrict__ pos, int K, uint32_t x) {
  if (L > 0) return block_search<false>(level, bt.nl, K, bt.stride, x, [&](int m) { return pos[m]; });
  int lo = 0, hi = K;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (pos[m] >= x) hi = m; else lo = m + 1;
  }
  return lo;
}

template <bool STORE>
__global__ __launch_bounds__(kProfileThreads) void k_profile(ProfileArgs A) {
  extern __shared__ unsigned long long profile_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int B = A.bins, L = A.lds_anchors, G = A.n_groups;
  const int track = (int)blockIdx.x;
  unsigned long long* l_sum = profile_lds;
  unsigned long long* l_sumsq = l_sum + (STORE ? 0 : B);
  unsigned long long* l_obs = l_sumsq + (STORE ? 0 : B);
  uint32_t* l_pos = reinterpret_cast<uint32_t*>(l_obs + (STORE ? 0 : B));
  uint32_t* l_less = l_pos + (STORE ? 0 : B);
  uint32_t* l_eq = l_less + (STORE ? 0 : B);
  uint32_t* vec = l_eq + (STORE ? 0 : B);
  uint32_t* part = vec + (size_t)wave * 2 * B;
  uint32_t* diff = part + B;
  uint32_t* tab = vec + (size_t)kProfileWaves * 2 * B;       // [group][level]

  const int64_t* __restrict__ off = A.anchor_off + (int64_t)track * G;
  {                           // everything up to the staged positions starts at 0
    uint32_t* words = reinterpret_cast<uint32_t*>(profile_lds);
    const int n_words = (int)(tab - words);
    for (int k = tid; k < n_words; k += kProfileThreads) words[k] = 0u;
  }
  for (int64_t k = tid; k < (int64_t)G * L; k += kProfileThreads) {
    const int lv = (int)(k % L), g = (int)(k / L);
    const int64_t b = off[g];
    const int K = (int)(off[g + 1] - b);
    const BlockTable bt = block_table(K, L);
    tab[k] = lv < bt.nl ? A.pos[b + min(K - 1, (lv + 1) * bt.stride - 1)] : 0u;
  }
  __syncthreads();
  if constexpr (!STORE) {
    for (int b = tid; b < B; b += kProfileThreads) l_obs[b] = (unsigned long long)A.obs[(int64_t)track * B + b];
    __syncthreads();
  }

  const int64_t w = A.bin_size, R = A.reach;
  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  for (int i = i0 + wave; i < i1; i += kProfileWaves) {
    uint32_t mn = UINT32_MAX, mx = 0u;                  // the bins this lane touched: [mn, mx]
    for (int g = 0; g < G; ++g) {
      const int64_t a0 = off[g];                        // (uniform)
      const int K = (int)(off[g + 1] - a0);
      if (K == 0) continue;
      int n;
      const uint2* __restrict__ seg = list_at(A.lists, i, g, G, n);
      const uint32_t* __restrict__ P = A.pos + a0;
      const uint8_t* __restrict__ M = A.minus + a0;
      const uint32_t* level = tab + (int64_t)g * L;
      const BlockTable bt = block_table(K, max(L, 1));
      // the segments that can meet an anchor lie between the first anchor's window and the last one's
      const int64_t first = (int64_t)P[0] - R, last = (int64_t)P[K - 1] + R;
      for (int j = lane; j < n; j += kWave) {
        const uint2 sg = seg[j];
        int64_t s = (int64_t)sg.x, e = (int64_t)sg.y;
        if (A.midpoints) { s = profile_midpoint(s, e); e = s + 1; }
        if (s > last) break;                            // (starts ascend: the lanes behind this one break too)
        if (e <= first) continue;
        const int64_t hi = profile_reach_hi(e, R);
        for (int k = profile_first_anchor(level, L, bt, P, K, profile_reach_lo(s, R)); k < K; ++k) {
          const int64_t a = (int64_t)P[k];
          if (a >= hi) break;
          ProfilePiece p;
          if (!profile_piece(s, e, a, M[k] != 0, w, R, p)) continue;
          atomicAdd(&part[p.fb], p.first);
          if (p.lb > p.fb) {
            atomicAdd(&part[p.lb], p.last);
            if (p.lb > p.fb + 1) { atomicAdd(&diff[p.fb + 1], 1u); atomicSub(&diff[p.lb], 1u); }
          }
          mn = min(mn, (uint32_t)p.fb);
          mx = max(mx, (uint32_t)p.lb);
        }
      }
    }
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    if (mn == UINT32_MAX) continue;                     // no base of this list in a window of the track
    wave_fence();
    uint32_t carry = 0u;
    for (int base = (int)(mn & ~(uint32_t)(kWave - 1)); base <= (int)mx; base += kWave) {
      const int b = base + lane;
      const bool in = b >= (int)mn && b <= (int)mx;
      const uint32_t d = in ? diff[b] : 0u;
      const uint32_t whole = carry + wave_incl_sum_u32(d, lane);
      carry = (uint32_t)__builtin_amdgcn_readlane((int)whole, kWave - 1);
      unsigned long long v = 0ull;
      if (in) {
        v = (unsigned long long)part[b] + (unsigned long long)w * (unsigned long long)whole;
        part[b] = 0u;
        diff[b] = 0u;
      }
      if (v == 0ull) continue;
      if constexpr (STORE) {
        A.out[((int64_t)i * A.n_tracks + track) * B + b] = v;
      } else {
        null_words_count(v, l_obs[b], [&](NullWord x, unsigned long long y) {
          if (x == kNullSum) atomicAdd(&l_sum[b], y);
          else if (x == kNullSumsq) atomicAdd(&l_sumsq[b], y);
          else atomicAdd(&(x == kNullPos ? l_pos : x == kNullLess ? l_less : l_eq)[b], (uint32_t)y);
        });
      }
    }
    wave_fence();
  }

  if constexpr (!STORE) {
    __syncthreads();
    for (int b = tid; b < B; b += kProfileThreads) {
      const uint32_t np = l_pos[b];
      if (np == 0u) continue;
      null_words_flush(A.out + ((int64_t)track * B + b) * kNullWords, np, l_sum[b], l_sumsq[b], l_less[b], l_eq[b]);
    }
  }
}

}  // namespace gat
