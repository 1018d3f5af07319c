// gat_local_windows.h -- what the launches of k_local (gat_local.h) decide on the host: the LDS a window of W bins takes, the
// widest window that fits, and the windows of a call -- W consecutive bins of one (track, contig) and the slice of the track
// that reaches into them; windows no interval reaches into are left out (every value there is 0).  Plain code -- no
// intrinsic, no runtime call -- so that all of it runs (and is checked: tests/host/local_windows_check.cpp) without a device.
#pragma once
#include <stdint.h>
#include <vector>
#include "gat_types.h"

namespace gat {

constexpr int kLocalThreads = 256;
constexpr int kLocalWaves = kLocalThreads / kWave;
constexpr int kLocalFoldBinBytes = 32;          // sum, sumsq (8 each), n_pos, n_less, n_eq, obs (4 each)
constexpr int kLocalWaveBinBytes = 8;           // part, diff

struct LocalWindow {
  int64_t lo;                 // first base of the window
  int64_t out;                // track * total_bins + the index of its first bin
  int64_t a0;                 // the first interval of the track's contig that reaches into it, in annos
  int32_t K;                  // intervals that do, >= 1
  int32_t contig;
  int32_t nb;                 // bins, 1 .. window_bins
  int32_t pad;
};

// dynamic LDS of a launch: (sum[W], sumsq[W] | n_pos[W], n_less[W], n_eq[W], obs[W])  part[waves][W], diff[waves][W]  l_s[L], l_e[L]
inline size_t local_lds_bytes(int64_t W, int64_t L, bool store) {
  return (size_t)W * (store ? 0 : kLocalFoldBinBytes) + (size_t)W * kLocalWaveBinBytes * kLocalWaves + (size_t)L * 8;
}
// the widest window a workgroup's LDS holds beside L staged pieces
inline int64_t local_max_window(int64_t lds, int64_t L) {
  return (lds - 1024 - L * 8) / (kLocalFoldBinBytes + kLocalWaveBinBytes * kLocalWaves);
}

// The windows of n_tracks x C normalized lists annos[anno_off[t * C + c] .. anno_off[t * C + c + 1]) over C contigs of
// bin_off[c + 1] - bin_off[c] bins of bin_size: appended to win, track by track, contig by contig, ascending; a0 counts from
// anno_off[0].  Coordinates are below 2^32: bins beyond that get no window.  false: 2^31 - 1 windows or more.
template <class Seg>
inline bool local_build_windows(const Seg* annos, const int64_t* anno_off, int32_t n_tracks, int32_t C, int64_t bin_size,
                                const int64_t* bin_off, int64_t W, std::vector<LocalWindow>& win) {
  const int64_t total = bin_off[C], reach = (((int64_t)1 << 32) + bin_size - 1) / bin_size;
  for (int32_t t = 0; t < n_tracks; ++t)
    for (int32_t c = 0; c < C; ++c) {
      const Seg* a = annos + anno_off[(int64_t)t * C + c];
      const int64_t n = anno_off[(int64_t)t * C + c + 1] - anno_off[(int64_t)t * C + c];
      const int64_t n_bins = bin_off[c + 1] - bin_off[c], eff = n_bins < reach ? n_bins : reach;
      if (n == 0 || eff == 0) continue;
      // (windows before the track's first base or behind its last hold nothing)
      const int64_t b_first = ((int64_t)a[0].start / bin_size) / W * W, b_last = ((int64_t)a[n - 1].end - 1) / bin_size + 1;
      const int64_t b_end = eff < b_last ? eff : b_last;
      int64_t k0 = 0;           // the first interval that ends beyond lo: ascends with the windows
      for (int64_t b = b_first; b < b_end; b += W) {
        const int32_t nb = (int32_t)(W < eff - b ? W : eff - b);
        const int64_t lo = b * bin_size, hi = lo + (int64_t)nb * bin_size;
        while (k0 < n && (int64_t)a[k0].end <= lo) ++k0;
        int64_t k1 = k0;
        while (k1 < n && (int64_t)a[k1].start < hi) ++k1;
        if (k1 == k0) continue;
        win.push_back({lo, (int64_t)t * total + bin_off[c] + b, anno_off[(int64_t)t * C + c] - anno_off[0] + k0, (int32_t)(k1 - k0), c, nb, 0});
      }
      if (win.size() >= (size_t)INT32_MAX) return false;
    }
  return true;
}

}  // namespace gat
