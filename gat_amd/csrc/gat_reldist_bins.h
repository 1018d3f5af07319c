// gat_reldist_bins.h -- the arithmetic of one (segment, flanking points) pair of k_reldist (gat_reldist.h), the area statistic
// of a list's histogram, and what its launches decide on the host.  The points of a (track, group) are K positions
// p_0 < ... < p_{K-1} in [0, 2^32 - 1]; a segment [s, e), e > s, stands for its midpoint m = s + (e - s) / 2 <= 2^32 - 2, and
// with j the first index whose point is > m -- the first point >= m + 1, which fits 32 bits -- it is INSIDE iff
// 1 <= j <= K - 1: p_{j-1} <= m < p_j.  Then d = min(m - p_{j-1}, p_j - m), gap = p_j - p_{j-1} >= 1 and its bin of B is
// min(B - 1, floor(2 d B / gap)): bin b covers the relative distances [b / 2B, (b + 1) / 2B), 0.5 itself goes to the last.
// Everything is unsigned 64-bit: 2 d B < 2^43.  Plain code for host and device -- no intrinsic, no runtime call -- so that
// all of it runs (and is checked: tests/host/reldist_bins_check.cpp) without a device.
#pragma once
#include <stdint.h>

namespace gat {

constexpr int kReldistThreads = 256;
constexpr int kReldistWaves = kReldistThreads / 64;
constexpr int kReldistMaxBins = 1024;           // GAT_RELDIST_MAX_BINS
constexpr int kReldistExtra = 3;                // GAT_RELDIST_EXTRA: area, inside, outside behind the bins
constexpr uint64_t kReldistAreaScale = 1000000; // GAT_RELDIST_AREA_SCALE
constexpr int kReldistFoldCellBytes = 36;       // sum, sumsq, obs (8 each), n_pos, n_less, n_eq (4 each)
constexpr int kReldistWaveBinBytes = 4;         // a wave's count of the bin

// the one base a segment [s, e), e > s, stands for
__host__ __device__ inline uint32_t reldist_midpoint(uint32_t s, uint32_t e) { return s + (e - s) / 2; }

// the bin of B of the midpoint m between its flanks lo <= m < hi
__host__ __device__ inline int reldist_bin(uint32_t m, uint32_t lo, uint32_t hi, int B) {
  const uint64_t below = (uint64_t)(m - lo), above = (uint64_t)(hi - m), gap = (uint64_t)(hi - lo);
  const uint64_t d = below < above ? below : above, num = 2 * d * (uint64_t)B;
  // (gap fits 32 bits; where the numerator does too -- every gap below 2^21 -- the division is the 32-bit one)
  const uint64_t b = (num >> 32) == 0 ? (uint64_t)((uint32_t)num / (uint32_t)gap) : num / gap;
  return b < (uint64_t)(B - 1) ? (int)b : B - 1;
}

// one term of D = sum_{b < B} |B * C_b - (b + 1) * n|, C_b the inside segments of the bins 0 .. b, n all of them:
// C_b <= n < 2^31 and b + 1 <= B <= 1024, so neither product passes 2^41
__host__ __device__ inline uint64_t reldist_area_term(uint64_t C, uint64_t n, int b, int B) {
  const uint64_t x = (uint64_t)B * C, y = (uint64_t)(b + 1) * n;
  return x > y ? x - y : y - x;
}

// floor(D * 10^6 / (n B^2)), the area between the list's ECDF over the bins and the uniform one in parts per million; 0 where
// n == 0.  M = n B^2 < 2^51 and D <= M (every term is at most B n): r = 1000 D < 2^61; with r = q M + t, t < M,
// 10^6 D / M = 1000 q + 1000 t / M and 1000 t < 2^61: exact, and no 128-bit division (there is none on the device).
__host__ __device__ inline uint64_t reldist_area(uint64_t D, uint64_t n, int B) {
  static_assert(kReldistAreaScale == 1000 * 1000, "the route takes the scale in two factors of 1000");
  if (n == 0) return 0;
  const uint64_t M = n * (uint64_t)B * (uint64_t)B, r = D * 1000;
  return (r / M) * 1000 + ((r % M) * 1000) / M;
}

// dynamic LDS of a launch: (sum[W], sumsq[W], obs[W] | n_pos[W], n_less[W], n_eq[W])  hist[waves][B]  tab[G][L], W = B + 3
__host__ __device__ inline int64_t reldist_lds_bytes(int64_t B, int64_t L, int64_t n_groups, bool store) {
  return (B + kReldistExtra) * (store ? 0 : kReldistFoldCellBytes) + B * kReldistWaveBinBytes * kReldistWaves + n_groups * L * 4;
}
// The positions of a (track, group) the search finds in LDS: at most `knob`, no more than the longest (track, group) of the call
// holds, and what the LDS of a compute unit (`lds` bytes, also the most a workgroup can have) takes beside the bins without
// costing a workgroup: the table never takes the compute unit below the workgroups (at most its 8 of 4 waves, 1 KB of slack
// each) it holds without one -- 0: the searches run in global memory
__host__ __device__ inline int64_t reldist_lds_points(int64_t knob, int64_t longest, int64_t lds, int64_t B, int64_t n_groups) {
  const int64_t bins = reldist_lds_bytes(B, 0, n_groups, false);
  int64_t n = lds / (bins + 1024);
  n = n < 8 ? n : 8;
  const int64_t room = n > 0 ? lds / n - 1024 - bins : 0;
  const int64_t fit = room > 0 ? room / ((n_groups > 1 ? n_groups : 1) * 4) : 0;
  int64_t L = knob < longest ? knob : longest;
  L = L < fit ? L : fit;
  return L > 0 ? L : 0;
}

}  // namespace gat
