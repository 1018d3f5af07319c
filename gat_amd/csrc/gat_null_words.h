// gat_null_words.h -- the sampled null of one tested cell, as gat_sample_bin_enrichment (a (track, bin): gat_local.h),
// gat_sample_pair_enrichment (a pair of tracks: gat_pairs.h) and gat_sample_geneset_enrichment (a term: gat_geneset.h) reduce
// it: over the S samples of a range, of the cell's value v >= 0 in a sample, five 64-bit words against the caller's obs >= 0
// (GAT_LOCAL_WORDS, GAT_PAIR_WORDS, GAT_GENESET_WORDS of include/gat_mi355.h):
//
//   n_pos (v > 0)   sum (of v)   sumsq (of v * v)   n_less (v < obs)   n_eq (v == obs)
//
// The (samples x cells) matrix is never formed.  A kernel meets only the samples with v > 0: it classifies each
// (null_words_count) into partial sums kept where it chooses -- LDS, registers, the result itself -- and adds a partial sum to
// the cell's words with 64-bit integer atomics (null_words_flush).  A partial sum has one owner and integer adds commute, so
// no split of the work and no order of arrival can change a bit.  The samples with v == 0 are counted at the very end,
// k_null_finish, from n_pos and S: n_less += (S - n_pos) * [0 < obs], n_eq += (S - n_pos) * [obs == 0].
#pragma once
#include "gat_device.h"

namespace gat {

constexpr int kNullWords = 5;
enum NullWord { kNullPos = 0, kNullSum = 1, kNullSumsq = 2, kNullLess = 3, kNullEq = 4 };

// one sample's v > 0 against o: add(word, x) is called for n_pos, sum, sumsq and for the one of n_less, n_eq that counts it
template <class Add>
__device__ __forceinline__ void null_words_count(unsigned long long v, unsigned long long o, Add add) {
  add(kNullPos, 1ull);
  add(kNullSum, v);
  add(kNullSumsq, v * v);
  if (v < o) add(kNullLess, 1ull);
  else if (v == o) add(kNullEq, 1ull);
}

// a partial sum with n_pos > 0 into the five words of its cell
__device__ __forceinline__ void null_words_flush(unsigned long long* cell, unsigned long long n_pos, unsigned long long sum,
                                                 unsigned long long sumsq, unsigned long long n_less, unsigned long long n_eq) {
  atomicAdd(cell + kNullPos, n_pos);
  atomicAdd(cell + kNullSum, sum);
  atomicAdd(cell + kNullSumsq, sumsq);
  if (n_less) atomicAdd(cell + kNullLess, n_less);
  if (n_eq) atomicAdd(cell + kNullEq, n_eq);
}

// the samples whose value is 0, which no kernel counted: S - n_pos of them per cell
__global__ __launch_bounds__(256) void k_null_finish(unsigned long long* out, const long long* __restrict__ obs, int64_t n, unsigned long long S) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  unsigned long long* o = out + k * kNullWords;
  const unsigned long long zeros = S - o[kNullPos];
  const long long ob = obs[k];
  if (ob > 0) o[kNullLess] += zeros;
  else if (ob == 0) o[kNullEq] += zeros;
}

}  // namespace gat
