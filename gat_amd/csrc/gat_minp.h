// gat_minp.h -- Westfall and Young's step-down minP adjusted p-values (in the formulation of Ge, Dudoit and Speed 2003,
// "Resampling-based multiple testing for microarray data analysis") read off the count matrix of a run: column i of the
// matrix is what EVERY annotation scored on the same sampled segment list, i.e. one draw from the joint null distribution
// of the family.  With T(r, x) the integer AnnotatorResult._two_sided turns into a p-value (getTwoSidedPValue,
// gat/Engine.pyx:1543-1576; pvalue = T / S),
//
//   n_less = #{i : row_r[i] < x},  n_eq = #{i : row_r[i] == x}
//   idx = 1                                                 if n_less == S
//       = S - (n_less - [n_eq > 0 and n_less > 0] + 1)      if x > mean_r
//       = n_less + n_eq                                     otherwise
//   T = max(1, idx)
//
// k_minp_rank writes K[r][i] = T(r, row_r[i]) -- every sample scored against its own row -- and k_minp_step walks the rows
// in the order o_R .. o_1 of (k_obs, row index), keeps q[i] = min over the rows seen so far of K[.][i], and counts per row
// c[o_j] = #{i : q_j[i] <= k_obs[o_j]}.  Everything is an integer; the running maximum and the division stay on the host.
//
// k_minp_rank: one workgroup per row.  The row's keys (stats_key: order of the keys == order of the doubles; -0.0 is keyed
// as 0.0, which compares equal to it as a double) are sorted by a least-significant-digit radix sort, 4 bits a pass:
// thread t owns the t-th contiguous chunk of the row, counts its chunk's digits into its OWN 16 LDS counters (no atomics),
// one scan over the 16 x 256 counters in (digit, thread) order gives every (digit, thread) its first output slot, and the
// thread scatters its chunk in order -- which is what makes the pass stable.  A digit in which all keys of the row agree
// is skipped (one OR-reduction of key ^ key[0] in front): counts are small integers held as doubles, their low mantissa
// digits are all zero, and 5 to 7 of the 16 passes remain.  A row of up to GAT_MINP_LDS_SAMPLES samples is sorted in LDS
// (two key buffers), a longer one in two global scratch rows of the workgroup.  n_less and n_eq of a sample are then the
// lower and upper bound of its key in the sorted row.
//
// k_minp_step: one thread per sample, lanes on consecutive samples (coalesced 4-byte loads of a row of K); per row one
// ballot + popcount and ONE vector atomic add per wave with a sample at or below the row's k_obs.
#pragma once
#include "gat_device.h"
#include "gat_stats.h"       // stats_key

namespace gat {

constexpr int kMinpThreads = 256;
constexpr int kMinpWaves = kMinpThreads / kWave;
constexpr int kMinpDigitBits = 4, kMinpDigits = 1 << kMinpDigitBits;
constexpr int kMinpHistWords = kMinpDigits * kMinpThreads;               // one counter per (digit, thread)
constexpr int kMinpMiscWords = 16;                                       // the waves' key differences (4 x 8 bytes), their scan totals (4 words)
constexpr int kMinpLdsFixed = (kMinpHistWords + kMinpMiscWords) * 4;     // bytes in front of the key buffers; a multiple of 16
constexpr int kMinpKeyBytes = 16;                                        // LDS per sample behind it: two 8-byte key buffers
constexpr int kMinpRankGrid = 512;                                       // workgroups of k_minp_rank at the most (each owns two scratch rows)
constexpr int kMinpStepUnroll = 4;

struct MinpRankArgs {
  const int64_t* counts;      // [row][S] 8-byte slots: int64, or IEEE double bits for rows flagged in is_double
  int64_t row_stride;
  int32_t S, n_rows;          // n_rows: rows of this batch
  const int32_t* rows;        // per batch row: the row of the matrix
  const uint8_t* is_double;   // per row of the matrix
  const double* means;        // per row of the matrix: AnnotatorResult.expected
  int32_t* K;                 // [batch row][S]
  unsigned long long* sort_scratch;   // [workgroup][2][S]; only where the keys do not fit LDS
  int32_t skip_passes;        // != 0: a digit in which all keys of the row agree is not sorted by
};

struct MinpStepArgs {
  const int32_t* K;           // [batch row][S], rows in o_R .. o_1 order
  int32_t S, n_rows;
  const int32_t* kobs;        // per batch row
  uint32_t* c;                // per batch row; zero before the call's first batch
  int32_t* q;                 // S: the running minimum, carried from batch to batch
  int32_t first;              // != 0: the call's first batch, q starts at +inf
};

__device__ __forceinline__ unsigned long long minp_key(double d) { return stats_key(d == 0.0 ? 0.0 : d); }

// T(r, x) from the two counts (the header's formula)
__device__ __forceinline__ int32_t minp_t(int32_t n_less, int32_t n_eq, int32_t S, bool above_mean) {
  int32_t idx;
  if (n_less == S) idx = 1;
  else if (above_mean) idx = S - (n_less - ((n_eq > 0 && n_less > 0) ? 1 : 0) + 1);
  else idx = n_less + n_eq;
  return idx > 1 ? idx : 1;
}

template <bool IN_LDS>
__global__ __launch_bounds__(kMinpThreads) void k_minp_rank(MinpRankArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* hist = lds;                                                         // [digit][thread]
  unsigned long long* wave_diff = reinterpret_cast<unsigned long long*>(lds + kMinpHistWords);   // [wave]
  uint32_t* wave_sum = lds + kMinpHistWords + 2 * kMinpWaves;                   // [wave]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int S = A.S;
  unsigned long long* keys;                                                     // two buffers of S keys, one behind the other
  if constexpr (IN_LDS) keys = reinterpret_cast<unsigned long long*>(lds + kMinpHistWords + kMinpMiscWords);
  else keys = A.sort_scratch + (int64_t)blockIdx.x * 2 * (int64_t)S;
  const int64_t chunk = ((int64_t)S + kMinpThreads - 1) / kMinpThreads;
  const int c0 = (int)(tid * chunk < (int64_t)S ? tid * chunk : (int64_t)S);
  const int c1 = (int)(c0 + chunk < (int64_t)S ? c0 + chunk : (int64_t)S);
  for (int b = blockIdx.x; b < A.n_rows; b += gridDim.x) {
    const int row = A.rows[b];
    const int64_t* __restrict__ src = A.counts + (int64_t)row * A.row_stride;
    const bool dbl = A.is_double[row] != 0;
    const double mean = A.means[row];
    auto value = [&](int i) -> double { const int64_t v = src[i]; return dbl ? __longlong_as_double(v) : (double)v; };
    // the keys, and the bits in which any two of them differ
    const unsigned long long key0 = minp_key(value(0));
    unsigned long long diff = 0ull;
    for (int i = tid; i < S; i += kMinpThreads) {
      const unsigned long long k = minp_key(value(i));
      keys[i] = k;
      diff |= k ^ key0;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) diff |= __shfl_xor(diff, m);
    if (lane == 0) wave_diff[wave] = diff;
    __syncthreads();
    diff = 0ull;
#pragma unroll
    for (int w = 0; w < kMinpWaves; ++w) diff |= wave_diff[w];
    if (!A.skip_passes) diff = ~0ull;
    int cur = 0;                                                                // the buffer that holds the keys
    for (int shift = 0; shift < 64; shift += kMinpDigitBits) {
      if (((diff >> shift) & (unsigned long long)(kMinpDigits - 1)) == 0ull) continue;      // (the same in every thread)
      const unsigned long long* from = keys + (cur ? (int64_t)S : 0);
      unsigned long long* to = keys + (cur ? 0 : (int64_t)S);
#pragma unroll
      for (int d = 0; d < kMinpDigits; ++d) hist[d * kMinpThreads + tid] = 0u;             // (a thread's own counters)
      for (int i = c0; i < c1; ++i) hist[((int)(from[i] >> shift) & (kMinpDigits - 1)) * kMinpThreads + tid] += 1u;
      __syncthreads();
      // exclusive scan over the counters in (digit, thread) order: a thread takes 16 consecutive ones
      uint32_t v[kMinpDigits], sum = 0u;
#pragma unroll
      for (int q = 0; q < kMinpDigits / 4; ++q) {
        const uint4 x = reinterpret_cast<const uint4*>(hist)[tid * (kMinpDigits / 4) + q];
        v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        sum += x.x + x.y + x.z + x.w;
      }
      const uint32_t incl = wave_incl_sum_u32(sum, lane);
      if (lane == kWave - 1) wave_sum[wave] = incl;
      __syncthreads();
      uint32_t run = incl - sum;
#pragma unroll
      for (int w = 0; w < kMinpWaves; ++w) run += w < wave ? wave_sum[w] : 0u;
#pragma unroll
      for (int q = 0; q < kMinpDigits / 4; ++q) {
        uint4 x;
        x.x = run; run += v[4 * q];
        x.y = run; run += v[4 * q + 1];
        x.z = run; run += v[4 * q + 2];
        x.w = run; run += v[4 * q + 3];
        reinterpret_cast<uint4*>(hist)[tid * (kMinpDigits / 4) + q] = x;
      }
      __syncthreads();
      for (int i = c0; i < c1; ++i) {                                           // in the chunk's order: the pass is stable
        const unsigned long long k = from[i];
        uint32_t* slot = &hist[((int)(k >> shift) & (kMinpDigits - 1)) * kMinpThreads + tid];
        const uint32_t pos = *slot;
        *slot = pos + 1u;
        if (pos < (uint32_t)S) to[pos] = k;                                     // (always: the counters add up to S)
      }
      __syncthreads();
      cur ^= 1;
    }
    // every sample against its own sorted row
    const unsigned long long* sorted = keys + (cur ? (int64_t)S : 0);
    int32_t* __restrict__ out = A.K + (int64_t)b * (int64_t)S;
    for (int i = tid; i < S; i += kMinpThreads) {
      const double x = value(i);
      const unsigned long long k = minp_key(x);
      int lo = 0, hi = S;
      while (lo < hi) {                                                         // first position with a key >= k
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < k) lo = mid + 1; else hi = mid;
      }
      const int n_less = lo;
      hi = S;
      while (lo < hi) {                                                         // first position with a key > k
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] <= k) lo = mid + 1; else hi = mid;
      }
      out[i] = minp_t(n_less, lo - n_less, S, x > mean);
    }
    __syncthreads();                                                            // (the next row takes the buffers)
  }
}

__global__ __launch_bounds__(kMinpThreads) void k_minp_step(MinpStepArgs A) {
  const int64_t i = (int64_t)blockIdx.x * kMinpThreads + threadIdx.x;
  const bool valid = i < (int64_t)A.S;
  const int lane = threadIdx.x & (kWave - 1);
  const int32_t* __restrict__ col = A.K + (valid ? i : 0);
  const int32_t* __restrict__ kobs = A.kobs;
  uint32_t* __restrict__ c = A.c;
  const int64_t S = A.S;
  int32_t q = (valid && !A.first) ? A.q[i] : INT32_MAX;
  auto step = [&](int b, int32_t k) {
    q = k < q ? k : q;
    const uint64_t m = __ballot(valid && q <= kobs[b]);
    if (lane == 0 && m != 0ull) atomicAdd(&c[b], (uint32_t)__popcll(m));
  };
  int b = 0;
  for (; b + kMinpStepUnroll <= A.n_rows; b += kMinpStepUnroll) {               // the loads of four rows in flight together
    int32_t k[kMinpStepUnroll];
#pragma unroll
    for (int u = 0; u < kMinpStepUnroll; ++u) k[u] = valid ? col[(int64_t)(b + u) * S] : INT32_MAX;
#pragma unroll
    for (int u = 0; u < kMinpStepUnroll; ++u) step(b + u, k[u]);
  }
  for (; b < A.n_rows; ++b) step(b, valid ? col[(int64_t)b * S] : INT32_MAX);
  if (valid) A.q[i] = q;
}

}  // namespace gat
