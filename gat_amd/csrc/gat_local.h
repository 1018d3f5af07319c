// gat_local.h -- where along the genome a list overlaps an annotation track: per bin of bin_size bases, formed where the
// lists are (gat_list_bin_overlaps, gat_sample_bin_enrichment).  For a normalized list L and a normalized track A of one
// contig and bin b < n_bins of it
//
//   v(L, A, b) = |L n A n [b * bin, (b + 1) * bin)|        0 <= v <= bin <= 2^31
//
// and over the samples of a range, per (track, bin), the five words of gat_null_words.h against the caller's obs.  The
// (samples x tracks x bins) matrix is never formed.
//
// A workgroup (256 threads, 4 waves) owns a WINDOW of W consecutive bins of one (track, contig) and a run of the lists of
// that contig.  It stages what the search for the first annotation interval starts in -- the window's slice of the track (the
// K intervals that reach into it, found by the host): all of them when K <= lds_pieces, else the last end of each block of
// `stride` intervals (block_table / block_search, gat_lists.h) -- and, when it folds, the window's obs, clamped to 32 bits (a
// value is at most 2^31: a larger obs compares like 2^32 - 1).  Windows no interval reaches into are not launched: v is 0.
//
// A WAVE takes one list at a time and owns a private vector in LDS: per bin a 32-bit sum of the pieces that cover the bin
// in part, and a 32-bit difference array of "covered whole" (+1 at the first whole bin of a piece, -1 at its last bin), as
// k_coverage has it -- a piece over many bins costs four adds.  L n A is disjoint, so a bin is covered whole by at most one
// piece and then by nothing else: v = part + bin * whole <= bin, and no 32-bit word can overflow.  The wave finds the first
// segment that reaches into the window -- into the part of it between the slice's first start and last end, which is all a
// segment can share with the track there -- (coverage_first_reaching), its lanes stride over the segments; a lane finds its
// first annotation interval with one search, walks the overlapping ones, clips each piece to the window and adds it with
// LDS atomics (two lanes may meet in a bin).  The lanes keep the range of bins they touched.  When the list is through, the
// wave sweeps that range only -- a list that touched nothing costs no sweep --, scans the difference array, forms v, clears
// the words behind it, and either STORES v (one owner per (list, track, bin): a plain store into an output the caller zeroed)
// or FOLDS it into the workgroup's per-bin accumulators in LDS: n_pos, n_less, n_eq (32 bits: at most one a list, the run is
// below 2^31) and sum, sumsq (64 bits) -- for v > 0 only.  At the end the workgroup adds the bins with n_pos > 0 to the
// result: consecutive lanes, consecutive bins.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_coverage.h"     // coverage_first_reaching
#include "gat_local_windows.h"
#include "gat_null_words.h"

namespace gat {

struct LocalArgs {
  ListSet lists;              // n_lists x n_groups of them, every one normalized
  int32_t n_lists;
  int32_t n_groups;
  int32_t lists_per_block;
  int32_t window_bins;        // W
  int32_t lds_pieces;         // L
  int32_t span32;             // W * bin_size <= 2^32: offsets inside a window divide in 32 bits
  int64_t bin_size;
  int64_t list_stride;        // STORE: n_tracks * total_bins, the words of a list
  const LocalWindow* win;     // gridDim.x of them
  const uint2* annos;
  const long long* obs;       // FOLD: [n_tracks][total_bins]
  unsigned long long* out;    // STORE: [n_lists][n_tracks][total_bins]; FOLD: [n_tracks][total_bins][kNullWords]
};

template <bool STORE>
__global__ __launch_bounds__(kLocalThreads) void k_local(LocalArgs A) {
  extern __shared__ unsigned long long local_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int W = A.window_bins, L = A.lds_pieces;
  unsigned long long* l_sum = local_lds;
  unsigned long long* l_sumsq = l_sum + (STORE ? 0 : W);
  uint32_t* l_pos = reinterpret_cast<uint32_t*>(l_sumsq + (STORE ? 0 : W));
  uint32_t* l_less = l_pos + (STORE ? 0 : W);
  uint32_t* l_eq = l_less + (STORE ? 0 : W);
  uint32_t* l_obs = l_eq + (STORE ? 0 : W);
  uint32_t* vec = l_obs + (STORE ? 0 : W);
  uint32_t* part = vec + (size_t)wave * 2 * W;
  uint32_t* diff = part + W;
  uint32_t* l_s = vec + (size_t)kLocalWaves * 2 * W;
  uint32_t* l_e = l_s + L;

  const LocalWindow win = A.win[blockIdx.x];
  const int nb = win.nb, K = win.K;
  const int64_t bin = A.bin_size;
  const int64_t lo = win.lo, hi = lo + (int64_t)nb * bin;
  const uint2* __restrict__ T = A.annos + win.a0;
  const BlockTable bt = block_table(K, L);
  const int stride = bt.stride, nl = bt.nl;
  // what a segment can share with the slice lies between the slice's first start and its last end: the segments are searched and
  // walked there, not over the whole window (a sparse track: a few hundred bases of a window of many thousands)
  const int64_t lo_s = max(lo, (int64_t)T[0].x), hi_s = min(hi, (int64_t)T[K - 1].y);

  {                           // everything up to the staged pieces starts at 0
    uint32_t* words = reinterpret_cast<uint32_t*>(local_lds);
    const int n_words = (int)((l_s - words));
    for (int k = tid; k < n_words; k += kLocalThreads) words[k] = 0u;
  }
  for (int t = tid; t < nl; t += kLocalThreads) {
    const uint2 v = T[min(K - 1, (t + 1) * stride - 1)];
    l_s[t] = v.x;
    l_e[t] = v.y;
  }
  __syncthreads();
  if constexpr (!STORE) {
    for (int b = tid; b < nb; b += kLocalThreads) {
      const long long o = A.obs[win.out + b];
      l_obs[b] = o > (long long)UINT32_MAX ? UINT32_MAX : (uint32_t)o;
    }
    __syncthreads();
  }

  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  // list (i, contig) as list_at finds it, with what does not depend on i read once and the length of the wave's next list on
  // its way while this one is worked on: a list that shares nothing with the slice is a chain of dependent reads and little else
  const bool csr = A.lists.csr != nullptr;
  const int64_t G = A.n_groups;
  const int n_at = csr ? 0 : A.lists.n_index[win.contig];
  const int64_t seg_at = csr ? 0 : (int64_t)A.lists.c_off[win.contig];
  auto length_of = [&](int i) -> int {
    if (i >= i1) return 0;
    return csr ? (int)(A.lists.csr[i * G + win.contig + 1] - A.lists.csr[i * G + win.contig]) : A.lists.n_arr[(int64_t)i * A.lists.n_stride + n_at];
  };
  int n_next = length_of(i0 + wave);
  for (int i = i0 + wave; i < i1; i += kLocalWaves) {
    const int n = n_next;
    n_next = length_of(i + kLocalWaves);
    const uint2* __restrict__ seg = csr ? A.lists.seg + A.lists.csr[i * G + win.contig] : A.lists.seg + (int64_t)i * A.lists.seg_stride + seg_at;
    const int j0 = coverage_first_reaching(seg, n, lo_s, lane);
    uint32_t mn = UINT32_MAX, mx = 0u;                // the bins this lane touched: [mn, mx]
    int j = j0 + lane;
    uint2 sg = j < n ? seg[j] : make_uint2(0u, 0u);
    while (j < n) {
      const int jn = j + kWave;                       // (the next round's segment is on its way while this one is searched)
      const uint2 nx = jn < n ? seg[jn] : make_uint2(0u, 0u);
      const int64_t s = (int64_t)sg.x, e = (int64_t)sg.y;
      if (s >= hi_s) break;                           // (starts ascend: the lanes behind this one break too)
      const int64_t cs = s > lo_s ? s : lo_s, ce = e < hi_s ? e : hi_s;
      sg = nx;
      j = jn;
      if (ce <= cs) continue;
      // the first interval that ends beyond cs; every one from there that starts below ce shares a piece with [cs, ce)
      int k = block_search<true>(l_e, nl, K, stride, (uint32_t)cs, [&](int m) { return T[m].y; });
      for (; k < K; ++k) {
        uint32_t ts, te;
        if (stride == 1) { ts = l_s[k]; te = l_e[k]; }
        else { const uint2 iv = T[k]; ts = iv.x; te = iv.y; }
        if ((int64_t)ts >= ce) break;
        const int64_t ps = (int64_t)ts > cs ? (int64_t)ts : cs, pe = (int64_t)te < ce ? (int64_t)te : ce;
        if (pe <= ps) continue;
        const int64_t rs = ps - lo, re = pe - lo;
        int fb, lb;
        if (A.span32) { fb = (int)((uint32_t)rs / (uint32_t)bin); lb = (int)((uint32_t)(re - 1) / (uint32_t)bin); }
        else { fb = (int)(rs / bin); lb = (int)((re - 1) / bin); }
        if (fb == lb) {
          atomicAdd(&part[fb], (uint32_t)(re - rs));
        } else {
          atomicAdd(&part[fb], (uint32_t)((int64_t)(fb + 1) * bin - rs));
          atomicAdd(&part[lb], (uint32_t)(re - (int64_t)lb * bin));
          if (lb > fb + 1) { atomicAdd(&diff[fb + 1], 1u); atomicSub(&diff[lb], 1u); }
        }
        mn = min(mn, (uint32_t)fb);
        mx = max(mx, (uint32_t)lb);
      }
    }
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    if (mn == UINT32_MAX) continue;                   // nothing of this list in the window
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
        v = (unsigned long long)part[b] + (unsigned long long)bin * (unsigned long long)whole;
        part[b] = 0u;
        diff[b] = 0u;
      }
      if (v == 0ull) continue;
      if constexpr (STORE) {
        A.out[(int64_t)i * A.list_stride + win.out + b] = v;
      } else {
        null_words_count(v, (unsigned long long)l_obs[b], [&](NullWord w, unsigned long long x) {
          if (w == kNullSum) atomicAdd(&l_sum[b], x);
          else if (w == kNullSumsq) atomicAdd(&l_sumsq[b], x);
          else atomicAdd(&(w == kNullPos ? l_pos : w == kNullLess ? l_less : l_eq)[b], (uint32_t)x);
        });
      }
    }
    wave_fence();
  }

  if constexpr (!STORE) {
    __syncthreads();
    for (int b = tid; b < nb; b += kLocalThreads) {
      const uint32_t np = l_pos[b];
      if (np == 0u) continue;
      null_words_flush(A.out + (win.out + b) * kNullWords, np, l_sum[b], l_sumsq[b], l_less[b], l_eq[b]);
    }
  }
}

}  // namespace gat
