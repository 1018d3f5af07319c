// gat_pairs.h -- which annotation tracks the segments of a list hit TOGETHER, counted where the lists are (gat_list_pair_hits,
// gat_sample_pair_enrichment).  A_t is track t, normalized per group (sorted, disjoint, none empty; adjacent ones allowed),
// q = [s, e), e > s, a segment of group g:
//
//   hit(q, t) = 1 iff j < K and A_t[j].start < e,  j = the first index with A_t[j].end > s       (bookended: no hit)
//   c(L, i, j) = the segments q of L, over all its groups, with hit(q, i) and hit(q, j)            i <= j
//
// and over the samples of a range, per pair, the five words of gat_null_words.h against the caller's obs.  The (samples x
// pairs) matrix is never formed.  The lists are taken in any order and may overlap themselves: every segment counts on its
// own; segments with e <= s are skipped.
//
// A workgroup (256 threads, 4 waves) owns a TILE of 64 x 64 tracks -- blocks (I, J), I <= J (gat_pairs_tiles.h) -- and a run
// of lists.  It takes one list at a time, all its groups; its waves stride over the list's segments in chunks of 64.
// SEARCH: LANE = SEGMENT.  The wave walks the tracks of block I -- the track, its K intervals and where they lie are uniform,
// scalar reads -- and every lane searches the track for its own segment: the lanes of a probe read the one list, a few cache
// lines, not 64 lists.  (The first level of the search -- the last end of each of up to L blocks of the track's intervals, per
// group -- is staged in LDS once per workgroup, [group][track][level]: lanes at different levels, different banks; the search
// ends in global memory: block_table, gat_lists.h.)  A lane ORs bit t into its 64-bit hit mask of the block when its segment
// hits track t.  Block J gives a second mask the same way, searched by the lanes whose first mask is not empty; a diagonal
// tile has one.
// COUNT: LANE = TRACK.  For every segment of the chunk with both masks set -- found by __ballot, its masks read with readlane,
// wave-uniform -- and every set bit b of its mask J -- a scalar loop -- the lanes whose own bit is set in its mask I add 1 to
// cnt[b][lane], the list's 32-bit count of the pair in LDS (an LDS atomic: another wave may meet it there; on the diagonal
// only lanes <= b add, the pairs with j >= i).  The cost of a segment is a search per track plus the set bits of mask J.
// When the list is through and any pair was touched, thread (wave w, lane a) sweeps the slots (a, w + 4 k), k < 16: a count
// c > 0 is cleared and either STORED (one owner per (list, pair): a plain store into an output the caller zeroed) or FOLDED
// into the result: 64-bit integer atomicAdd of 1, c, c * c and of the comparison with obs -- one owner per (list, pair), added
// once; integer adds commute, so neither the tile, nor the run, nor the batches, nor the order of arrival can change a bit.
// (Partial sums of a run kept in registers -- 16 slots x five words a thread, 190 VGPRs -- were measured and gained nothing: the
// adds are as many as the pairs a list touches, few beside its searches.)
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_pairs_tiles.h"
#include "gat_null_words.h"

namespace gat {

struct PairsArgs {
  ListSet lists;              // n_lists x n_groups of them, in any order
  int32_t n_lists;
  int32_t n_groups;
  int32_t n_tracks;
  int32_t lists_per_block;
  int32_t lds_pieces;         // L: the dynamic LDS is pairs_lds_bytes(L, n_groups)
  const uint2* annos;
  const int64_t* anno_csr;    // [n_tracks * n_groups + 1], track-major, from 0
  const long long* obs;       // FOLD: [P]
  unsigned long long* out;    // STORE: [n_lists][P]; FOLD: [P][kNullWords]
};

// a track of one group: its K intervals and where the search for them starts (level: the track's row of the table)
struct PairsTrack {
  const uint2* T;
  const uint32_t* level;
  int K, stride, nl;
};
__device__ __forceinline__ PairsTrack pairs_track(const PairsArgs& A, const uint32_t* tab, int track, int slot, int g) {
  const int64_t b = A.anno_csr[(int64_t)track * A.n_groups + g];
  PairsTrack t = {A.annos + b, tab + ((int64_t)g * kPairsTileTracks + slot) * A.lds_pieces,
                  (int)(A.anno_csr[(int64_t)track * A.n_groups + g + 1] - b), 1, 0};
  if (A.lds_pieces > 0) { const BlockTable bt = block_table(t.K, A.lds_pieces); t.stride = bt.stride; t.nl = bt.nl; }
  else t.stride = t.K;
  return t;
}
// hit([s, e), the track), K > 0: block_search (gat_lists.h), the start read where the end was found
__device__ __forceinline__ bool pairs_hit(const PairsTrack& t, int L, uint32_t s, uint32_t e) {
  int a = 0;
  if (L > 0) {
    int b = t.nl;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (t.level[m] > s) b = m; else a = m + 1;
    }
    if (a == t.nl) return false;
    if (t.stride == 1) return t.T[a].x < e;
  } else if (t.T[t.K - 1].y <= s) {
    return false;
  }
  int lo = a * t.stride, hi = (t.K < lo + t.stride ? t.K : lo + t.stride) - 1;     // (T[hi].end > s)
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (t.T[m].y > s) hi = m; else lo = m + 1;
  }
  return t.T[lo].x < e;
}

// the lane's segment [s, e) against the n tracks of a block, first track `track0`, whose rows of the table begin at `slot0`:
// bit t set where it hits track0 + t.  (All lanes of the wave come here; `live` says whether this one has a segment to ask for.)
__device__ __forceinline__ unsigned long long pairs_block_mask(const PairsArgs& A, const uint32_t* tab, int track0, int n, int slot0, int g,
                                                               bool live, uint32_t s, uint32_t e) {
  unsigned long long mask = 0ull;
  for (int t = 0; t < n; ++t) {
    const PairsTrack tr = pairs_track(A, tab, track0 + t, slot0 + t, g);      // (uniform)
    if (tr.K == 0) continue;
    if (live && pairs_hit(tr, A.lds_pieces, s, e)) mask |= 1ull << t;
  }
  return mask;
}
__device__ __forceinline__ unsigned long long pairs_readlane_u64(unsigned long long v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

template <bool STORE>
__global__ __launch_bounds__(kPairsThreads) void k_pairs(PairsArgs A) {
  extern __shared__ uint32_t pairs_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int G = A.n_groups, L = A.lds_pieces;
  const int64_t T = A.n_tracks, P = pairs_count(T);
  int I, J;
  pairs_tile_at((int64_t)blockIdx.x, pairs_blocks(T), I, J);
  const bool diag = I == J;
  uint32_t* cnt = pairs_lds;                       // [b][a]: consecutive lanes, consecutive words
  uint32_t* tab = pairs_lds + kPairsTileSlots;     // [group][track of the tile: block I's 64, block J's 64][level]

  for (int k = tid; k < kPairsTileSlots; k += kPairsThreads) cnt[k] = 0u;
  for (int64_t k = tid; k < (int64_t)G * L * kPairsTileTracks; k += kPairsThreads) {
    const int lv = (int)(k % L), slot = (int)(k / L % kPairsTileTracks), g = (int)(k / L / kPairsTileTracks);
    const int64_t track = (int64_t)(slot < kPairsBlock ? I : J) * kPairsBlock + (slot & (kPairsBlock - 1));
    uint32_t v = 0u;
    if (track < T) {
      const int64_t b = A.anno_csr[track * G + g];
      const int K = (int)(A.anno_csr[track * G + g + 1] - b);
      const BlockTable bt = block_table(K, L);
      if (lv < bt.nl) v = A.annos[b + min(K - 1, (lv + 1) * bt.stride - 1)].y;
    }
    tab[k] = v;
  }
  __syncthreads();

  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  const int n_i = (int)min((int64_t)kPairsBlock, T - (int64_t)I * kPairsBlock), n_j = (int)min((int64_t)kPairsBlock, T - (int64_t)J * kPairsBlock);
  for (int i = i0; i < i1; ++i) {
    int any = 0;
    for (int g = 0; g < G; ++g) {
      int n;
      const uint2* __restrict__ Q = list_at(A.lists, i, g, G, n);
      for (int j0 = wave * kWave; j0 < n; j0 += kPairsWaves * kWave) {
        const int j = j0 + lane;
        const uint2 sg = j < n ? Q[j] : make_uint2(0u, 0u);
        const bool live = sg.y > sg.x;
        const unsigned long long mi = pairs_block_mask(A, tab, I * kPairsBlock, n_i, 0, g, live, sg.x, sg.y);
        if (__ballot(mi != 0ull) == 0ull) continue;
        const unsigned long long mj = diag ? mi : pairs_block_mask(A, tab, J * kPairsBlock, n_j, kPairsBlock, g, mi != 0ull, sg.x, sg.y);
        unsigned long long todo = __ballot(mi != 0ull && mj != 0ull);
        if (todo == 0ull) continue;
        any = 1;
        while (todo != 0ull) {                      // a segment that hits in both blocks: lanes are tracks now
          const int l = __ffsll((long long)todo) - 1;
          todo &= todo - 1ull;
          const bool mine = (pairs_readlane_u64(mi, l) >> lane) & 1ull;
          unsigned long long m = pairs_readlane_u64(mj, l);
          while (m != 0ull) {
            const int b = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            if (mine && (!diag || lane <= b)) atomicAdd(&cnt[b * kPairsBlock + lane], 1u);
          }
        }
      }
    }
    if (!__syncthreads_or(any)) continue;           // no pair of the tile in this list
#pragma unroll 1                                    // (unrolled, the sixteen slots' addresses and words are live at once)
    for (int k = 0; k < kPairsSlotsPerThread; ++k) {
      const int e = tid + kPairsThreads * k;
      const uint32_t c = cnt[e];
      if (c == 0u) continue;
      cnt[e] = 0u;
      const int64_t pk = pairs_slot(I, J, lane, wave + kPairsWaves * k, T);
      if (pk < 0) continue;
      if constexpr (STORE) {
        A.out[(int64_t)i * P + pk] = (unsigned long long)c;
      } else {
        const unsigned long long o = (unsigned long long)A.obs[pk];
        unsigned long long* cell = A.out + pk * kNullWords;
        null_words_count((unsigned long long)c, o, [&](NullWord w, unsigned long long x) { atomicAdd(cell + w, x); });
      }
    }
    __syncthreads();
  }
}

}  // namespace gat
