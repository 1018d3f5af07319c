// gat_geneset.h -- which GENE SETS (terms) the segments of a list reach, counted where the lists are (gat_list_geneset_hits,
// gat_sample_geneset_enrichment).  The genes of a group are flattened by the host into PIECES: sorted, disjoint, none empty
// (adjacent ones allowed); piece j carries members(j), the ascending gene ids that cover it, a CSR over the pieces of all groups.
// q = [s, e), e > s, a segment of group g:
//
//   j0 = the first piece with end > s,  j1 = the first piece with start >= e          (bookended: j1 == j0, no hit)
//   hit(q, .) = the members of pieces j0 .. j1 - 1 = members[member_off[j0] .. member_off[j1])  -- ONE contiguous range
//   H(L) = the genes hit by any segment of L, all its groups;   c(L, t) = |H(L) n M_t|
//
// and over the samples of a range, per term, the five words of gat_null_words.h against the caller's obs.  The lists are taken
// in any order and may overlap themselves; segments with e <= s are skipped.
//
// TWO KERNELS, a bitmap of n_genes bits per list between them (global scratch, [list][words]):
//
// k_geneset_hits: a workgroup (256 threads) takes a run of lists one at a time, all groups, and keeps the list's bitmap in LDS.
// LANE = SEGMENT: a lane makes two searches over the piece ENDS of the group -- block_search (gat_lists.h), first level in LDS,
// [group][level], staged once per workgroup -- for j0 and for k = the first piece with end >= e (j1 = k + [start(k) < e]: the
// pieces are disjoint, so the starts need no table of their own), reads the two member offsets and ORs the bits of its range
// into the bitmap with LDS atomics.  A range longer than kGenesetLaneRange entries -- a segment over a gene desert's neighbour,
// a nest 40 deep -- is not walked by its lane: the wave takes such ranges one after the other (__ballot, readlane), 64 entries
// a step, so that no lane holds the wave for longer than kGenesetLaneRange steps.  The bitmap goes out with plain, coalesced
// stores: one owner per (list, word).
//
// k_geneset_terms: a workgroup owns a TILE of up to 256 terms and a run of lists.  Per list it stages the bitmap in LDS, then
// LANE = TERM for the terms of at most kGenesetLaneTerm genes (the median term has ten): the lane walks its own list and adds
// up the bits; a longer term (the tail: hundreds to all genes) is strided by a whole wave, 64 genes a step, the tile's long
// terms dealt round-robin to the four waves, reduced with shuffles.  The thread that owns the term then has c: STORED (one
// owner per (list, term)) or FOLDED into the thread's five partial words, kept in registers over the run and added to the
// result once at its end with 64-bit integer atomics: one owner per (run, term); integer adds commute, so neither the tile,
// nor the run, nor the batches, nor the order of arrival can change a bit.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_null_words.h"

namespace gat {

constexpr int kGenesetThreads = 256;
constexpr int kGenesetWaves = kGenesetThreads / kWave;
constexpr int kGenesetMaxGenes = 262144;                 // GAT_GENESET_MAX_GENES: a bitmap of 32 KB
constexpr int kGenesetMaxTermTile = kGenesetThreads;     // a thread owns a term of the tile
constexpr int kGenesetLaneRange = 16;                    // member entries a lane walks on its own
constexpr int kGenesetLaneTerm = 64;                     // genes of a term a lane walks on its own
constexpr int64_t kGenesetTableBudget = 32 * 1024;       // bytes of the searches' first level beside the bitmap: 64 KB a workgroup at most

// words of a list's bitmap (at least one, so that every list has a row)
__host__ __device__ inline int64_t geneset_bitmap_words(int64_t n_genes) { return n_genes > 0 ? (n_genes + 31) / 32 : 1; }
// L: the knob's, as far as n_groups tables fit the budget
__host__ __device__ inline int64_t geneset_lds_pieces(int64_t knob, int64_t n_groups) {
  const int64_t fit = kGenesetTableBudget / 4 / (n_groups > 1 ? n_groups : 1);
  return knob < 0 ? 0 : (knob < fit ? knob : fit);
}

struct GenesetHitsArgs {
  ListSet lists;              // n_groups lists an entity, in any order
  int32_t list_begin;         // the launch takes lists [list_begin, list_begin + n_lists)
  int32_t n_lists;
  int32_t n_groups;
  int32_t lists_per_block;
  int32_t lds_pieces;         // L: the dynamic LDS is (bm_words + n_groups * L) * 4
  int32_t bm_words;
  const uint2* pieces;
  const int64_t* piece_csr;   // [n_groups + 1], from 0
  const int64_t* member_off;  // [n_pieces + 1], from 0
  const int32_t* members;
  uint32_t* bitmaps;          // [n_lists][bm_words]: row i is list list_begin + i
};

struct GenesetTermsArgs {
  const uint32_t* bitmaps;    // [n_lists][bm_words]
  int32_t list_begin;         // STORE: row i goes to out[list_begin + i]
  int32_t n_lists;
  int32_t lists_per_block;
  int32_t bm_words;
  int32_t term_tile;          // terms of a workgroup, 1 .. kGenesetMaxTermTile
  int32_t n_terms;
  const int64_t* term_off;    // [n_terms + 1], from 0
  const int32_t* term_genes;
  const long long* obs;       // FOLD: [n_terms]
  unsigned long long* out;    // STORE: [all lists][n_terms]; FOLD: [n_terms][kNullWords]
};

// first j in [0, K) with end(j) > x (UPPER) / >= x, K: none; nl == 0: no first level in LDS
template <bool UPPER>
__device__ __forceinline__ int geneset_search(const uint2* __restrict__ T, const uint32_t* level, int nl, int K, int stride, uint32_t x) {
  if (nl > 0) return block_search<UPPER>(level, nl, K, stride, x, [&](int m) { return T[m].y; });
  int lo = 0, hi = K;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    const uint32_t v = T[m].y;
    if (UPPER ? v > x : v >= x) hi = m; else lo = m + 1;
  }
  return lo;
}
__device__ __forceinline__ int64_t geneset_readlane_i64(int64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void geneset_set(uint32_t* bm, int32_t gene) { atomicOr(&bm[gene >> 5], 1u << (gene & 31)); }

__global__ __launch_bounds__(kGenesetThreads) void k_geneset_hits(GenesetHitsArgs A) {
  extern __shared__ uint32_t geneset_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int G = A.n_groups, L = A.lds_pieces, W = A.bm_words;
  uint32_t* bm = geneset_lds;
  uint32_t* tab = geneset_lds + W;                 // [group][level]

  for (int w = tid; w < W; w += kGenesetThreads) bm[w] = 0u;
  for (int64_t k = tid; k < (int64_t)G * L; k += kGenesetThreads) {
    const int lv = (int)(k % L), g = (int)(k / L);
    const int64_t b = A.piece_csr[g];
    const int K = (int)(A.piece_csr[g + 1] - b);
    const BlockTable bt = block_table(K, L);
    tab[k] = lv < bt.nl ? A.pieces[b + min(K - 1, (lv + 1) * bt.stride - 1)].y : 0u;
  }
  __syncthreads();

  const int i0 = (int)blockIdx.x * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  for (int i = i0; i < i1; ++i) {
    for (int g = 0; g < G; ++g) {
      const int64_t pb = A.piece_csr[g];
      const int K = (int)(A.piece_csr[g + 1] - pb);
      if (K == 0) continue;
      int n;
      const uint2* __restrict__ Q = list_at(A.lists, (int64_t)A.list_begin + i, g, G, n);
      const uint2* __restrict__ T = A.pieces + pb;
      const uint32_t* level = tab + (int64_t)g * L;
      int stride = 1, nl = 0;
      if (L > 0) { const BlockTable bt = block_table(K, L); stride = bt.stride; nl = bt.nl; }
      for (int q0 = wave * kWave; q0 < n; q0 += kGenesetWaves * kWave) {
        const int q = q0 + lane;
        const uint2 sg = q < n ? Q[q] : make_uint2(0u, 0u);
        int64_t m0 = 0, m1 = 0;
        if (sg.y > sg.x) {
          const int p0 = geneset_search<true>(T, level, nl, K, stride, sg.x);
          if (p0 < K) {
            const int k = geneset_search<false>(T, level, nl, K, stride, sg.y);
            const int p1 = k == K ? K : k + (T[k].x < sg.y ? 1 : 0);
            m0 = A.member_off[pb + p0];
            m1 = A.member_off[pb + p1];
          }
        }
        const bool wide = m1 - m0 > (int64_t)kGenesetLaneRange;
        if (!wide)
          for (int64_t m = m0; m < m1; ++m) geneset_set(bm, A.members[m]);
        unsigned long long todo = __ballot(wide);
        while (todo != 0ull) {                      // a long range: the wave's, 64 entries a step
          const int l = __ffsll((long long)todo) - 1;
          todo &= todo - 1ull;
          const int64_t a0 = geneset_readlane_i64(m0, l), a1 = geneset_readlane_i64(m1, l);
          for (int64_t m = a0 + lane; m < a1; m += kWave) geneset_set(bm, A.members[m]);
        }
      }
    }
    __syncthreads();
    uint32_t* row = A.bitmaps + (int64_t)i * W;
    for (int w = tid; w < W; w += kGenesetThreads) { row[w] = bm[w]; bm[w] = 0u; }
    __syncthreads();
  }
}

template <bool STORE>
__global__ __launch_bounds__(kGenesetThreads) void k_geneset_terms(GenesetTermsArgs A) {
  extern __shared__ uint32_t geneset_lds[];
  __shared__ uint32_t cbuf[kGenesetMaxTermTile];
  __shared__ int long_idx[kGenesetMaxTermTile];
  __shared__ int n_long;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int W = A.bm_words;
  uint32_t* bm = geneset_lds;
  const int64_t tile0 = (int64_t)blockIdx.x * A.term_tile;
  const int64_t t = tile0 + tid;
  const bool own = tid < A.term_tile && t < (int64_t)A.n_terms;
  const int64_t b0 = own ? A.term_off[t] : 0, b1 = own ? A.term_off[t + 1] : 0;
  const bool is_long = b1 - b0 > (int64_t)kGenesetLaneTerm;
  if (tid == 0) n_long = 0;
  __syncthreads();
  if (is_long) long_idx[atomicAdd(&n_long, 1)] = tid;     // (in any order: a long term's count comes back to its owner by slot)
  __syncthreads();
  const int nlong = n_long;
  const unsigned long long o = STORE || !own ? 0ull : (unsigned long long)A.obs[t];      // (obs >= 0)
  unsigned long long n_pos = 0ull, sum = 0ull, sumsq = 0ull, n_less = 0ull, n_eq = 0ull;

  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  for (int i = i0; i < i1; ++i) {
    const uint32_t* __restrict__ row = A.bitmaps + (int64_t)i * W;
    for (int w = tid; w < W; w += kGenesetThreads) bm[w] = row[w];
    __syncthreads();
    uint32_t c = 0u;
    if (!is_long)
      for (int64_t m = b0; m < b1; ++m) {
        const int32_t g = A.term_genes[m];
        c += (bm[g >> 5] >> (g & 31)) & 1u;
      }
    for (int k = wave; k < nlong; k += kGenesetWaves) {
      const int slot = long_idx[k];
      const int64_t a0 = A.term_off[tile0 + slot], a1 = A.term_off[tile0 + slot + 1];
      int part = 0;
      for (int64_t m = a0 + lane; m < a1; m += kWave) {
        const int32_t g = A.term_genes[m];
        part += (int)((bm[g >> 5] >> (g & 31)) & 1u);
      }
      for (int d = kWave / 2; d > 0; d >>= 1) part += __shfl_xor(part, d);
      if (lane == 0) cbuf[slot] = (uint32_t)part;
    }
    __syncthreads();                                // (the bitmap is read; the long terms' counts are there)
    if (is_long) c = cbuf[tid];
    if (c == 0u) continue;
    const unsigned long long v = (unsigned long long)c;
    if constexpr (STORE) {
      A.out[((int64_t)A.list_begin + i) * A.n_terms + t] = v;
    } else {                                        // (null_words_count's step, spelled out: through a callable the five leave the registers)
      n_pos += 1ull;
      sum += v;
      sumsq += v * v;
      if (v < o) n_less += 1ull;
      else if (v == o) n_eq += 1ull;
    }
  }
  if constexpr (!STORE) {
    if (n_pos == 0ull) return;
    null_words_flush(A.out + t * kNullWords, n_pos, sum, sumsq, n_less, n_eq);
  }
}

}  // namespace gat
