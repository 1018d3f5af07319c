// gat_metrics_tables.h -- the host side of k_metrics (gat_metrics.h): the workspace pieces of every group as the kernel
// searches them, and the two prefix tables it takes `inter` and the gap count from.  Plain host code -- no context, no
// runtime call -- so it runs (and is checked: tests/host/metrics_tables_check.cpp) without a device.
//
// Group g holds K = off[g + 1] - off[g] pieces, sorted and disjoint; pieces may be adjacent (normalize does not merge
// start == previous end).  Its prefix tables have K + 1 entries each, at off[g] + g:
//   cum[j]  = summed length of the pieces below j                         (cum[0] = 0, cum[K] = the group's bases)
//   gaps[j] = number of j' in 1..j with start[j'] > end[j' - 1]           (gaps[0] = 0)
// so the pieces lo..hi hold cum[hi + 1] - cum[lo] bases and gaps[hi] - gaps[lo] positive gaps lie between them.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/gat_mi355.h"

struct MetricsTables {
  std::vector<uint32_t> start, end, gaps;
  std::vector<unsigned long long> cum;
  std::vector<int32_t> off;              // n_groups + 1
};

// GAT_OK, or GAT_ERR_ARG with `err` naming what is wrong with ws_off or with the first list that is not normalized
inline int metrics_build_tables(const gat_segment* ws, const int64_t* ws_off, int64_t n_groups, MetricsTables& T, std::string& err) {
  char buf[256];
  if (ws_off[0] < 0) { err = "ws_off[0] < 0"; return GAT_ERR_ARG; }
  for (int64_t g = 0; g < n_groups; ++g)
    if (ws_off[g + 1] < ws_off[g]) {
      snprintf(buf, sizeof(buf), "ws_off decreases at group %lld", (long long)g);
      err = buf;
      return GAT_ERR_ARG;
    }
  const int64_t base = ws_off[0], total = ws_off[n_groups] - base;
  if (total + n_groups + 1 >= (int64_t)INT32_MAX) { err = "more than 2^31 workspace pieces"; return GAT_ERR_ARG; }
  if (total > 0 && ws == nullptr) { err = "NULL workspace with pieces"; return GAT_ERR_ARG; }
  T.start.resize((size_t)total);
  T.end.resize((size_t)total);
  T.gaps.resize((size_t)(total + n_groups));
  T.cum.resize((size_t)(total + n_groups));
  T.off.resize((size_t)n_groups + 1);
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t b = ws_off[g] - base, K = ws_off[g + 1] - ws_off[g];
    T.off[(size_t)g] = (int32_t)b;
    unsigned long long run = 0;
    uint32_t ngaps = 0;
    for (int64_t j = 0; j < K; ++j) {
      const gat_segment w = ws[base + b + j];
      if (w.end <= w.start || (j > 0 && w.start < ws[base + b + j - 1].end)) {
        snprintf(buf, sizeof(buf), "workspace list %lld is not normalized at piece %lld", (long long)g, (long long)j);
        err = buf;
        return GAT_ERR_ARG;
      }
      if (j > 0 && w.start > ws[base + b + j - 1].end) ++ngaps;
      T.start[(size_t)(b + j)] = w.start;
      T.end[(size_t)(b + j)] = w.end;
      T.cum[(size_t)(b + g + j)] = run;
      T.gaps[(size_t)(b + g + j)] = ngaps;
      run += (unsigned long long)(w.end - w.start);
    }
    T.cum[(size_t)(b + g + K)] = run;
    T.gaps[(size_t)(b + g + K)] = ngaps;
  }
  T.off[(size_t)n_groups] = (int32_t)total;
  return GAT_OK;
}
