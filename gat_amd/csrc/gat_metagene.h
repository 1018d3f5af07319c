// gat_metagene.h -- how the segments of a list are distributed along a class of SCALED features (genes, enhancers, CpG islands)
// and their flanks, formed where the lists are (gat_list_metagene, gat_sample_metagene_enrichment).  A feature is
// (fs, fe, sigma); every feature is stretched to Bb body bins, 5' to 3', with Bf flank bins of w bases on both sides
// (gat_metagene_bins.h has the conventions): B = 2 Bf + Bb bins, F = Bf * w.  For a normalized list L over the groups g and a
// feature track t
//
//   v(L, t, b) = sum over g, over features f of (t, g), over q in L_g of  #{ x in q : x in window(f), bin(x; f) = b }
//
// (GAT_METAGENE_MIDPOINTS: q replaced by its midpoint base), a base counting once per feature whose window holds it; and over
// the samples of a range, per (track, bin), the five words of gat_null_words.h against the caller's obs.  The (samples x tracks
// x bins) matrix is never formed.
//
// The ownership is k_profile's (gat_profile.h): a workgroup (256 threads, 4 waves) owns one feature TRACK and a run of lists; a
// WAVE takes one list at a time over ALL groups, with a private vector in LDS (part, diff); the lanes stride over the segments
// of (list, g).  Two things differ.  The features overlap and nest, so their ends do not ascend: a lane makes ONE search, for
// the first k with pm[k] + F > s on the prefix maximum of the ends, pm[k] = max(fe[0 .. k]) (built on the host) -- from the
// LDS image of pm where there is one (block_table / block_search, gat_lists.h), the search ending in global memory beyond L
// entries, all of it there with L == 0 -- then walks forward while fs[k] < e + F and passes over the features with
// fe[k] + F <= s: short features nested under a long one that reaches the segment are walked, not searched past.  And a body
// bin's width differs from feature to feature, so the difference array cannot carry "covered whole" for the body: the flanks
// use part + diff as k_profile does (a flank piece over many bins costs four adds), a body bin gets one add per bin touched
// (one or two as a rule; Bb where the segment swallows the feature), its edges stepped without a division (MetageneEdge).
// The list is disjoint, so one feature sends at most w bases into a flank bin and ceil(len / Bb) into a body bin: no word
// passes the bound the host refuses at 2^32.  The sweep behind a list, STORE and FOLD are k_profile's.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_metagene_bins.h"
#include "gat_null_words.h"

namespace gat {

struct MetageneArgs {
  ListSet lists;              // n_lists x n_groups of them, every one normalized
  int32_t n_lists;
  int32_t n_groups;
  int32_t n_tracks;
  int32_t lists_per_block;
  int32_t bins;               // B = 2 * flank_bins + body_bins
  int32_t body_bins;          // Bb
  int32_t flank_bins;         // Bf
  int32_t lds_features;       // L: the dynamic LDS is metagene_lds_bytes(B, L, n_groups, STORE)
  int32_t midpoints;          // GAT_METAGENE_MIDPOINTS
  int64_t flank_bin_size;     // w
  int64_t flank;              // F
  const uint32_t* fs;         // the features, ascending by (fs, fe, minus) per (track, group)
  const uint32_t* fe;
  const uint32_t* pm;         // pm[k] = max(fe[first of the (track, group) .. k])
  const uint8_t* minus;
  const int64_t* feat_off;    // [n_tracks * n_groups + 1], track-major, from 0
  const long long* obs;       // FOLD: [n_tracks][B]
  unsigned long long* out;    // STORE: [n_lists][n_tracks][B]; FOLD: [n_tracks][B][kNullWords]
};

// first k in [0, K) with pm[k] > x, K: none -- from the staged level (bt: its block_table) where there is one
__device__ __forceinline__ int metagene_first_feature(const uint32_t* level, int L, const BlockTable& bt, const uint32_t* __restrict__ pm, int K, uint32_t x) {
  if (L > 0) return block_search<true>(level, bt.nl, K, bt.stride, x, [&](int m) { return pm[m]; });
  int lo = 0, hi = K;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (pm[m] > x) hi = m; else lo = m + 1;
  }
  return lo;
}

template <bool STORE>
__global__ __launch_bounds__(kMetageneThreads) void k_metagene(MetageneArgs A) {
  extern __shared__ unsigned long long metagene_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int B = A.bins, L = A.lds_features, G = A.n_groups, Bb = A.body_bins, Bf = A.flank_bins;
  const int track = (int)blockIdx.x;
  unsigned long long* l_sum = metagene_lds;
  unsigned long long* l_sumsq = l_sum + (STORE ? 0 : B);
  unsigned long long* l_obs = l_sumsq + (STORE ? 0 : B);
  uint32_t* l_pos = reinterpret_cast<uint32_t*>(l_obs + (STORE ? 0 : B));
  uint32_t* l_less = l_pos + (STORE ? 0 : B);
  uint32_t* l_eq = l_less + (STORE ? 0 : B);
  uint32_t* vec = l_eq + (STORE ? 0 : B);
  uint32_t* part = vec + (size_t)wave * 2 * B;
  uint32_t* diff = part + B;
  uint32_t* tab = vec + (size_t)kMetageneWaves * 2 * B;      // [group][level]

  const int64_t* __restrict__ off = A.feat_off + (int64_t)track * G;
  {                           // everything up to the staged ends starts at 0
    uint32_t* words = reinterpret_cast<uint32_t*>(metagene_lds);
    const int n_words = (int)(tab - words);
    for (int k = tid; k < n_words; k += kMetageneThreads) words[k] = 0u;
  }
  for (int64_t k = tid; k < (int64_t)G * L; k += kMetageneThreads) {
    const int lv = (int)(k % L), g = (int)(k / L);
    const int64_t b = off[g];
    const int K = (int)(off[g + 1] - b);
    const BlockTable bt = block_table(K, L);
    tab[k] = lv < bt.nl ? A.pm[b + min(K - 1, (lv + 1) * bt.stride - 1)] : 0u;
  }
  __syncthreads();
  if constexpr (!STORE) {
    for (int b = tid; b < B; b += kMetageneThreads) l_obs[b] = (unsigned long long)A.obs[(int64_t)track * B + b];
    __syncthreads();
  }

  const int64_t w = A.flank_bin_size, F = A.flank;
  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  for (int i = i0 + wave; i < i1; i += kMetageneWaves) {
    uint32_t mn = UINT32_MAX, mx = 0u;                  // the bins this lane touched: [mn, mx]
    // what a piece puts into one flank: first and last bin in part, the bins between them covered whole
    auto add_flank = [&](const MetageneFlank& f) {
      if (f.fb < 0) return;
      atomicAdd(&part[f.fb], f.first);
      if (f.lb > f.fb) {
        atomicAdd(&part[f.lb], f.last);
        if (f.lb > f.fb + 1) { atomicAdd(&diff[f.fb + 1], 1u); atomicSub(&diff[f.lb], 1u); }
      }
      mn = min(mn, (uint32_t)f.fb);
      mx = max(mx, (uint32_t)f.lb);
    };
    for (int g = 0; g < G; ++g) {
      const int64_t a0 = off[g];                        // (uniform)
      const int K = (int)(off[g + 1] - a0);
      if (K == 0) continue;
      int n;
      const uint2* __restrict__ seg = list_at(A.lists, i, g, G, n);
      const uint32_t* __restrict__ FS = A.fs + a0;
      const uint32_t* __restrict__ FE = A.fe + a0;
      const uint32_t* __restrict__ PM = A.pm + a0;
      const uint8_t* __restrict__ M = A.minus + a0;
      const uint32_t* level = tab + (int64_t)g * L;
      const BlockTable bt = block_table(K, max(L, 1));
      // the segments that can meet a feature lie between the first window's start and the last window end of all
      const int64_t first = (int64_t)FS[0] - F, last = (int64_t)PM[K - 1] + F;
      for (int j = lane; j < n; j += kWave) {
        const uint2 sg = seg[j];
        int64_t s = (int64_t)sg.x, e = (int64_t)sg.y;
        if (A.midpoints) { s = profile_midpoint(s, e); e = s + 1; }
        if (s >= last) break;                           // (starts ascend: the lanes behind this one break too)
        if (e <= first) continue;
        const int64_t hi = metagene_reach_hi(e, F);
        uint32_t key;
        int k = metagene_reach_key(s, F, key) ? metagene_first_feature(level, L, bt, PM, K, key) : 0;
        for (; k < K; ++k) {
          const int64_t fs = (int64_t)FS[k];
          if (fs >= hi) break;
          const int64_t fe = (int64_t)FE[k];
          if (!metagene_reaches(s, fe, F)) continue;    // (a feature that ends before the segment, under one that does not)
          if (A.midpoints) {
            const int32_t b = metagene_bin(s, fs, fe, M[k] != 0, Bb, Bf, w);
            if (b < 0) continue;
            atomicAdd(&part[b], 1u);
            mn = min(mn, (uint32_t)b);
            mx = max(mx, (uint32_t)b);
            continue;
          }
          MetagenePiece p;
          if (!metagene_piece(s, e, fs, fe, M[k] != 0, Bb, Bf, w, p)) continue;
          add_flank(p.up);
          add_flank(p.down);
          if (p.body.fb < 0) continue;
          MetageneEdge E = p.body.edge;
          int64_t lo = p.body.oa;
          for (int b = p.body.fb; b <= p.body.lb; ++b) {              // the body offsets [lo, up) lie in body bin b
            const int64_t edge = metagene_edge_value(E), up = edge < p.body.ob ? edge : p.body.ob;
            if (up > lo) atomicAdd(&part[Bf + b], (uint32_t)(up - lo));
            lo = up;
            metagene_edge_next(E);
          }
          mn = min(mn, (uint32_t)(Bf + p.body.fb));
          mx = max(mx, (uint32_t)(Bf + p.body.lb));
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
      const uint32_t whole = carry + wave_incl_sum_u32(d, lane);    // (0 over the body: a flank's pair of marks lies in the flank)
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
    for (int b = tid; b < B; b += kMetageneThreads) {
      const uint32_t np = l_pos[b];
      if (np == 0u) continue;
      null_words_flush(A.out + ((int64_t)track * B + b) * kNullWords, np, l_sum[b], l_sumsq[b], l_less[b], l_eq[b]);
    }
  }
}

}  // namespace gat
