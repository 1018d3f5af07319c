// gat_coverage.h -- per-bin coverage of the sampled lists, formed where the lists are (gat_sample_coverage; stands in for
// computeSegmentDensityProfile, test/validate_randomization.py:212-247 of the reference, which walks the samples base by
// base on the host).  For every list (sample i, contig c) of a batch and every segment [s, e), e > s, of it:
//
//   bases[c][b]  += |[s, e) n [b * bin, (b + 1) * bin)|     b < n_bins[c]
//   outside[c]   += |[s, e) n [n_bins[c] * bin, inf)|
//   starts[c][b] += 1 where s lies in bin b;  ends[c][b] += 1 where e - 1 does (beyond the last bin: dropped)
//
// all in 64 bits.  No global atomic per segment: a workgroup owns a WINDOW of consecutive bins of one contig for a chunk
// of the batch's samples and keeps it in LDS -- per bin a 64-bit sum of the partial overlaps (a segment has at most two:
// its first and its last bin), a 32-bit difference array of "covers this bin whole" (+1 at the first whole bin, -1 at the
// segment's last bin), 32-bit starts and ends: 20 bytes a bin.  Its waves take the chunk's samples in turn; a wave finds
// the list's first segment that reaches into the window with a 64-ary search on the ends (normalized lists: starts and
// ends both ascend) and walks on until a start lies behind the window; lists that are neither sorted nor disjoint
// (SamplerSegments without isochore keys) are scanned whole.  Every segment is clipped to the window, so one that spans
// several windows is seen by each of them and nothing is carried from window to window.  At the end the workgroup scans
// the difference array, forms partial + bin * whole in 64 bits and adds the window to the result: consecutive lanes,
// consecutive bins, 64-bit integer atomicAdd, bins that stayed 0 skipped -- the sums do not depend on the order of arrival.
// The tail [n_bins * bin, inf) of a contig is a window of its own without bins: one sum per workgroup, one atomicAdd.
//
// The 32-bit words cannot overflow: the launch keeps (samples of a chunk) x (slots of a sample's slab) below 2^31.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"

namespace gat {

constexpr int kCoverageThreads = 512;
constexpr int kCoverageWaves = kCoverageThreads / kWave;
constexpr int kCoverageBinBytes = 20;

struct CoverageWindow {
  int64_t lo;                 // first base of the window (the tail: n_bins * bin, or 2^32 where that is beyond every coordinate)
  int64_t out;                // index of its first bin in bases / starts / ends
  int32_t contig;
  int32_t nb;                 // bins, 1 .. window_bins; 0: the contig's tail
};

struct CoverageArgs {
  ListSet lists;              // the batch's: n_samples x contigs of them
  int32_t n_samples;
  int32_t samples_per_block;
  int32_t window_bins;        // W: the LDS image is sized for it
  int32_t sorted;             // the lists are normalized: search; 0: scan
  int64_t bin_size;
  const CoverageWindow* win;  // gridDim.x of them
  unsigned long long* bases;
  unsigned long long* starts; // nullptr with ends: not wanted
  unsigned long long* ends;
  unsigned long long* outside;
};

// dynamic LDS of a launch: partial[W] (8 bytes), diff[W + 1 (+ 1: even)], starts[W], ends[W]
__host__ __device__ inline size_t coverage_lds_bytes(int64_t W) { return (size_t)W * 8 + (size_t)((W + 2) & ~(int64_t)1) * 4 + (size_t)W * 8; }

// first j in [0, n) with seg[j].y > lo (n: none), ends ascending: 64 probes a round, the range shrinks 64-fold
__device__ __forceinline__ int coverage_first_reaching(const uint2* __restrict__ seg, int n, int64_t lo, int lane) {
  int a = 0, b = n;           // every j < a ends at or below lo; b == n or seg[b] reaches beyond lo
  while (a < b) {
    const int step = (b - a + kWave - 1) / kWave;
    const int64_t idx = (int64_t)a + (int64_t)lane * step;
    const bool reaches = idx < b ? (int64_t)seg[idx].y > lo : true;
    const uint64_t m = __ballot(reaches);
    if (m == 0) { a += (kWave - 1) * step + 1; continue; }
    const int f = (int)__builtin_ctzll(m);
    const int64_t hit = (int64_t)a + (int64_t)f * step;
    if (hit < b) b = (int)hit;
    if (f > 0) a += (f - 1) * step + 1;
    else b = a;
  }
  return a;
}

__global__ __launch_bounds__(kCoverageThreads) void k_coverage(CoverageArgs A) {
  extern __shared__ unsigned long long cov_lds[];
  __shared__ unsigned long long s_outside;
  __shared__ uint32_t s_wave_sum[kCoverageWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int W = A.window_bins;
  unsigned long long* partial = cov_lds;
  uint32_t* diff = reinterpret_cast<uint32_t*>(partial + W);
  uint32_t* l_starts = diff + ((W + 2) & ~1);
  uint32_t* l_ends = l_starts + W;
  const CoverageWindow win = A.win[blockIdx.x];
  const int nb = win.nb;
  const int64_t bin = A.bin_size;
  const int64_t lo = win.lo;
  const int64_t hi = nb > 0 ? lo + (int64_t)nb * bin : (int64_t)1 << 40;
  if (nb > 0) {
    uint32_t* words = reinterpret_cast<uint32_t*>(cov_lds);
    const int n_words = (int)(coverage_lds_bytes(W) / 4);
    for (int k = tid; k < n_words; k += kCoverageThreads) words[k] = 0u;
  }
  if (tid == 0) s_outside = 0ull;
  __syncthreads();

  const int i0 = (int)blockIdx.y * A.samples_per_block;
  const int i1 = min(i0 + A.samples_per_block, A.n_samples);
  unsigned long long beyond = 0ull;
  // (always a sampler batch, so no group count; said aloud, the contig's offset and index are read once, not per sample)
  __builtin_assume(A.lists.csr == nullptr);
  for (int i = i0 + wave; i < i1; i += kCoverageWaves) {
    int n;
    const uint2* __restrict__ seg = list_at(A.lists, i, win.contig, 0, n);
    const int j0 = A.sorted ? coverage_first_reaching(seg, n, lo, lane) : 0;
    for (int j = j0 + lane; j < n; j += kWave) {
      const uint2 sg = seg[j];
      const int64_t s = (int64_t)sg.x, e = (int64_t)sg.y;
      if (A.sorted && s >= hi) break;                 // (starts ascend: the lanes behind this one break too)
      const int64_t cs = s > lo ? s : lo, ce = e < hi ? e : hi;
      if (e <= s || ce <= cs) continue;
      if (nb == 0) { beyond += (unsigned long long)(ce - cs); continue; }
      const int64_t rs = cs - lo, re = ce - lo;
      const int fb = (int)(rs / bin), lb = (int)((re - 1) / bin);
      if (fb == lb) {
        atomicAdd(&partial[fb], (unsigned long long)(re - rs));
      } else {
        atomicAdd(&partial[fb], (unsigned long long)((int64_t)(fb + 1) * bin - rs));
        atomicAdd(&partial[lb], (unsigned long long)(re - (int64_t)lb * bin));
        if (lb > fb + 1) { atomicAdd(&diff[fb + 1], 1u); atomicSub(&diff[lb], 1u); }
      }
      if (A.starts != nullptr) {
        if (cs == s) atomicAdd(&l_starts[fb], 1u);
        if (ce == e) atomicAdd(&l_ends[lb], 1u);
      }
    }
  }

  if (nb == 0) {
    if (beyond) atomicAdd(&s_outside, beyond);
    __syncthreads();
    if (tid == 0 && s_outside) atomicAdd(&A.outside[win.contig], s_outside);
    return;
  }
  __syncthreads();
  // the difference array -> whole-bin counts, in place: a thread owns a run of bins, the runs' sums are scanned
  const int run = (W + kCoverageThreads - 1) / kCoverageThreads;
  const int b0 = tid * run;
  uint32_t mine = 0;
  for (int k = 0; k < run; ++k) if (b0 + k < nb) mine += diff[b0 + k];
  const uint32_t incl = wave_incl_sum_u32(mine, lane);
  if (lane == kWave - 1) s_wave_sum[wave] = incl;
  __syncthreads();
  uint32_t whole = incl - mine;
  for (int w = 0; w < wave; ++w) whole += s_wave_sum[w];
  for (int k = 0; k < run; ++k)
    if (b0 + k < nb) { whole += diff[b0 + k]; diff[b0 + k] = whole; }
  __syncthreads();
  for (int b = tid; b < nb; b += kCoverageThreads) {
    const unsigned long long v = partial[b] + (unsigned long long)bin * (unsigned long long)diff[b];
    if (v) atomicAdd(&A.bases[win.out + b], v);
    if (A.starts != nullptr) {
      if (l_starts[b]) atomicAdd(&A.starts[win.out + b], (unsigned long long)l_starts[b]);
      if (l_ends[b]) atomicAdd(&A.ends[win.out + b], (unsigned long long)l_ends[b]);
    }
  }
}

}  // namespace gat
