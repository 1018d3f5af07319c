// gat_null_fold.h -- k_null_fold: a round of a count matrix folded, where gat_sample_and_count left it, into eight exact
// 64-bit words per (counter, track) row (GAT_NULL_FOLD_WORDS of include/gat_mi355.h):
//
//   n   sum (of v)   sumsq_lo, sumsq_hi (the 128-bit sum of v * v)   n_less (v < val)   n_eq (v == val)   min   max
//
// A run whose null distribution is deeper than a matrix that fits draws its samples in rounds into ONE buffer and folds
// each round into the same words (gat_amd.run(null_round_size=...)); the table is made from the words.  Everything is
// integer arithmetic: the host hands the row's val over as two integers -- `lt`, the smallest integer not below val clamped
// to [0, 2^63] (for an integer v, v < val is v < ceil(val)), and `eq`, val itself when it is an integer a slot can hold,
// else kNullFoldNoEq, which no v < 2^63 equals -- and v * v is the full 128-bit product, added with its carry.
//
// Launch: blockIdx.x = the row, blockIdx.y = the part of the row (gridDim.y parts of `chunk` samples).  A lane keeps its
// partial words in registers, the wave and then the workgroup reduce them, and thread 0 adds the workgroup's partial words
// to the row's with 64-bit integer atomics, as null_words_flush (gat_null_words.h) does: integer adds, min and max commute
// and a partial sum has one owner, so the words depend neither on the grid, nor on the cut of a row, nor on the order of
// arrival.  The low sumsq word is added with a returning atomic: the adder whose addition wraps it adds 1 to the high word
// -- the number of wraps is floor(total / 2^64) whatever the order.
// The matrix is read once, 16 bytes a lane and load where the part starts on a 16-byte boundary; the one slot in front of
// that boundary and the one behind the last pair are taken singly.
#pragma once
#include "gat_device.h"

namespace gat {

constexpr int kNullFoldWords = 8;
constexpr int kNullFoldThreads = 256;
constexpr unsigned long long kNullFoldNoEq = ~0ull;
enum NullFoldWord { kFoldN = 0, kFoldSum = 1, kFoldSumsqLo = 2, kFoldSumsqHi = 3, kFoldLess = 4, kFoldEq = 5, kFoldMin = 6, kFoldMax = 7 };

struct NullFoldArgs {
  const unsigned long long* counts;   // the first row of the launch
  int64_t row_stride;                 // slots between rows
  int64_t S;                          // slots of a row in use
  int64_t chunk;                      // slots per part
  const unsigned long long* lt;       // per row
  const unsigned long long* eq;
  unsigned long long* words;          // the first row's
};

// a lane's / wave's / workgroup's partial words
struct NullFoldPart {
  unsigned long long sum = 0, sq_lo = 0, sq_hi = 0, less = 0, eq = 0, mn = ~0ull, mx = 0;
  __device__ __forceinline__ void take(unsigned long long v, unsigned long long lt, unsigned long long e) {
    sum += v;
    const unsigned long long lo = v * v;
    sq_lo += lo;
    sq_hi += __umul64hi(v, v) + (sq_lo < lo ? 1ull : 0ull);
    less += v < lt ? 1ull : 0ull;
    eq += v == e ? 1ull : 0ull;
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  __device__ __forceinline__ void add(const NullFoldPart& o) {
    sum += o.sum;
    sq_lo += o.sq_lo;
    sq_hi += o.sq_hi + (sq_lo < o.sq_lo ? 1ull : 0ull);
    less += o.less;
    eq += o.eq;
    mn = o.mn < mn ? o.mn : mn;
    mx = o.mx > mx ? o.mx : mx;
  }
};

__device__ __forceinline__ NullFoldPart null_fold_wave(NullFoldPart p) {
  p.sum = (unsigned long long)wave_sum_i64((long long)p.sum);
  p.less = (unsigned long long)wave_sum_i64((long long)p.less);
  p.eq = (unsigned long long)wave_sum_i64((long long)p.eq);
  wave_sum_u128(p.sq_lo, p.sq_hi);
  p.mn = wave_min_u64(p.mn);
  p.mx = wave_max_u64(p.mx);
  return p;
}

__global__ __launch_bounds__(kNullFoldThreads) void k_null_fold(NullFoldArgs A) {
  const int64_t r = blockIdx.x;
  const int64_t b = (int64_t)blockIdx.y * A.chunk;
  const int64_t e = b + A.chunk < A.S ? b + A.chunk : A.S;
  if (b >= e) return;                                   // (more parts than the row has chunks)
  const unsigned long long* row = A.counts + r * A.row_stride;
  const unsigned long long lt = A.lt[r], eq = A.eq[r];
  const int tid = threadIdx.x;
  NullFoldPart p;
  // [b, e) = at most one slot in front of a 16-byte boundary, pairs, at most one slot behind them
  const int64_t head = (((uintptr_t)(row + b)) & 15) ? 1 : 0;
  const int64_t n_pairs = (e - b - head) >> 1;
  const ulonglong2* __restrict__ q = reinterpret_cast<const ulonglong2*>(row + b + head);
  if (head && tid == 0) p.take(row[b], lt, eq);
  if (tid == kNullFoldThreads - 1 && b + head + 2 * n_pairs < e) p.take(row[e - 1], lt, eq);
#pragma unroll 4
  for (int64_t i = tid; i < n_pairs; i += kNullFoldThreads) {
    const ulonglong2 v = q[i];
    p.take(v.x, lt, eq);
    p.take(v.y, lt, eq);
  }
  p = null_fold_wave(p);
  __shared__ unsigned long long s_part[kNullFoldThreads / 64][7];
  if ((tid & 63) == 0) {
    unsigned long long* s = s_part[tid >> 6];
    s[0] = p.sum; s[1] = p.sq_lo; s[2] = p.sq_hi; s[3] = p.less; s[4] = p.eq; s[5] = p.mn; s[6] = p.mx;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < kNullFoldThreads / 64; ++w) {
    const unsigned long long* s = s_part[w];
    NullFoldPart o;
    o.sum = s[0]; o.sq_lo = s[1]; o.sq_hi = s[2]; o.less = s[3]; o.eq = s[4]; o.mn = s[5]; o.mx = s[6];
    p.add(o);
  }
  unsigned long long* o = A.words + r * kNullFoldWords;
  atomicAdd(o + kFoldN, (unsigned long long)(e - b));
  atomicAdd(o + kFoldSum, p.sum);
  const unsigned long long before = atomicAdd(o + kFoldSumsqLo, p.sq_lo);
  const unsigned long long up = p.sq_hi + (before + p.sq_lo < before ? 1ull : 0ull);
  if (up) atomicAdd(o + kFoldSumsqHi, up);
  if (p.less) atomicAdd(o + kFoldLess, p.less);
  if (p.eq) atomicAdd(o + kFoldEq, p.eq);
  atomicMin(o + kFoldMin, p.mn);
  atomicMax(o + kFoldMax, p.mx);
}

// the words of rows nothing was folded into yet: zeros, min = 2^64 - 1
__global__ __launch_bounds__(256) void k_null_fold_reset(unsigned long long* words, int64_t n_words) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n_words) words[k] = (k & (kNullFoldWords - 1)) == kFoldMin ? ~0ull : 0ull;
}

}  // namespace gat
