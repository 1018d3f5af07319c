// gat_profile_bins.h -- the arithmetic of one (segment, anchor) pair of k_profile (gat_profile.h), and what its launches decide
// on the host.  An anchor is (a, sigma): a position a in [0, 2^32 - 1] and a strand sigma in {+1, -1}.  With w = bin_size,
// H = half_bins, R = H * w <= 2^31 and B = 2 H bins, the offset of base x is o = sigma * (x - a), x lies in the window iff
// -R <= o < R, and its bin is floor((o + R) / w): bin b covers the offsets [b * w - R, (b + 1) * w - R).  A plus anchor's
// window is [a - R, a + R), a minus anchor's (a - R, a + R].  Everything is 64-bit: a - R goes below 0 and a + R passes 2^32.
// Plain code for host and device -- no intrinsic, no runtime call -- so that all of it runs (and is checked:
// tests/host/profile_bins_check.cpp) without a device.
#pragma once
#include <stdint.h>

namespace gat {

constexpr int kProfileThreads = 256;
constexpr int kProfileWaves = kProfileThreads / 64;
constexpr int kProfileMaxBins = 1024;           // GAT_PROFILE_MAX_BINS
constexpr int kProfileFoldBinBytes = 36;        // sum, sumsq, obs (8 each), n_pos, n_less, n_eq (4 each)
constexpr int kProfileWaveBinBytes = 8;         // part, diff

// What the bases of [s, e) put into the bins of one anchor: the bins [fb, lb]; `first` bases into fb; when lb > fb, `last`
// bases into lb and w into every bin between them.
struct ProfilePiece {
  int32_t fb, lb;
  uint32_t first, last;
};

// [s, e), e > s, against the anchor (a, minus): false where no base of it lies in the window.  The clip is exact by strand;
// u = o + R runs over [us, ue), 0 <= us < ue <= 2 R <= 2^32, ascending in x for a plus anchor and descending for a minus one.
__host__ __device__ inline bool profile_piece(int64_t s, int64_t e, int64_t a, bool minus, int64_t w, int64_t R, ProfilePiece& p) {
  const int64_t lo = minus ? a - R + 1 : a - R, hi = lo + 2 * R;       // the window's bases [lo, hi)
  const int64_t cs = s > lo ? s : lo, ce = e < hi ? e : hi;
  if (ce <= cs) return false;
  const int64_t us = minus ? hi - ce : cs - lo, ue = minus ? hi - cs : ce - lo;
  // (us and ue - 1 are below 2^32 and w is at most 2^31: the divisions are 32-bit)
  const uint32_t fb = (uint32_t)us / (uint32_t)w, lb = (uint32_t)(ue - 1) / (uint32_t)w;
  p.fb = (int32_t)fb;
  p.lb = (int32_t)lb;
  if (fb == lb) {
    p.first = (uint32_t)(ue - us);
    p.last = 0u;
  } else {
    p.first = (uint32_t)((int64_t)(fb + 1) * w - us);
    p.last = (uint32_t)(ue - (int64_t)lb * w);
  }
  return true;
}

// the midpoint of [s, e): the one base GAT_PROFILE_MIDPOINTS counts
__host__ __device__ inline int64_t profile_midpoint(int64_t s, int64_t e) { return s + (e - s) / 2; }

// The anchors a segment [s, e) can meet, of either strand, have positions in [profile_reach_lo, profile_reach_hi): a plus
// anchor needs s - R < a <= e - 1 + R, a minus one s - R <= a < e - 1 + R.  (profile_piece drops the one at the edge that misses.)
__host__ __device__ inline uint32_t profile_reach_lo(int64_t s, int64_t R) { return s > R ? (uint32_t)(s - R) : 0u; }
__host__ __device__ inline int64_t profile_reach_hi(int64_t e, int64_t R) { return e + R; }

// dynamic LDS of a launch: (sum[B], sumsq[B], obs[B] | n_pos[B], n_less[B], n_eq[B])  part[waves][B], diff[waves][B]  tab[G][L]
__host__ __device__ inline int64_t profile_lds_bytes(int64_t B, int64_t L, int64_t n_groups, bool store) {
  return B * (store ? 0 : kProfileFoldBinBytes) + B * kProfileWaveBinBytes * kProfileWaves + n_groups * L * 4;
}
// how many workgroups of `bytes` of LDS (and 1 KB of slack each) a compute unit of `lds` bytes holds, at most its 8 of 4 waves
__host__ __device__ inline int64_t profile_workgroups_per_cu(int64_t lds, int64_t bytes) {
  const int64_t n = lds / (bytes + 1024);
  return n < 8 ? n : 8;
}
// The anchor positions of a (track, group) the search finds in LDS: at most `knob`, no more than the longest (track, group) of
// the call holds, and what the LDS of a compute unit (`lds` bytes, which is also the most a workgroup can have) takes beside
// the bins WITHOUT costing a workgroup: the table never takes the compute unit below the workgroups it holds without one
// (at B = 1024 the bins are 68 KB: one workgroup a compute unit instead of two was measured at 1.7 x the time) -- 0: the
// searches run in global memory
__host__ __device__ inline int64_t profile_lds_anchors(int64_t knob, int64_t longest, int64_t lds, int64_t B, int64_t n_groups) {
  const int64_t bins = profile_lds_bytes(B, 0, n_groups, false), n = profile_workgroups_per_cu(lds, bins);
  const int64_t room = n > 0 ? lds / n - 1024 - bins : 0;
  const int64_t fit = room > 0 ? room / ((n_groups > 1 ? n_groups : 1) * 4) : 0;
  int64_t L = knob < longest ? knob : longest;
  L = L < fit ? L : fit;
  return L > 0 ? L : 0;
}

}  // namespace gat
