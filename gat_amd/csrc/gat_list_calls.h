// gat_list_calls.h -- the entry points of libgat_mi355.so that reduce segment lists: the caller's own (gat_list_*) or the
// sampled lists of a problem where they lie (gat_sample, gat_sample_*).  Host code; part of gat_mi355.hip's translation unit
// (the one place that includes it, behind the batch seam it calls into), not a header for anybody else.
#pragma once

// ---- the entry points that read the sampled lists where they are: gat_sample / gat_sample_units copy them out, and
// gat_sample_coverage, gat_sample_metrics, gat_sample_distances, gat_sample_signal, gat_sample_bin_enrichment,
// gat_sample_pair_enrichment, gat_sample_geneset_enrichment, gat_sample_profile_enrichment, gat_sample_reldist_enrichment and gat_sample_metagene_enrichment put a kernel
// (gat_coverage.h, gat_metrics.h, gat_distance.h, gat_signal.h, gat_local.h, gat_pairs.h, gat_geneset.h, gat_profile.h, gat_reldist.h, gat_metagene.h) behind every batch.  They share the call's frame, the batch loop and the view of a batch's lists.

// A synchronous call's frame: refused while a call is in flight on the problem (P == nullptr: a call over the caller's own
// lists); the knobs are read once; body(kn, local) does the work.  Whatever the body returns, the stream is drained behind it:
// the device buffers of the call -- declared by the entry point BEFORE the frame, so destroyed after it -- go back to the
// process-wide pool, which hands an idle block to any context or stream, only when no kernel reads them any more.
template <class Body>
static int call_frame(gat_ctx* ctx, gat_problem* P, gat_stats* stats, Body body) {
  if (P && P->call.active) return set_err(ctx, GAT_ERR_ARG, "a call is in flight on this problem (its scratch is in use): gat_wait first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const Knobs kn = read_knobs(ctx);
  gat_stats local;
  memset(&local, 0, sizeof(local));
  const int rc = body(kn, local);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->stage_used = 0;
  if (stats) *stats = local;
  return rc;
}

// S samples in batches as the scratch takes them: after_batch(done, nb) behind every batch that passed its checks -- a batch
// that is laid out again (kRelayout) or failed never gets there, so nothing of it is seen twice -- and the batch is counted.
// (timed unless another problem's call in flight owns the context's per-kernel events)
template <class After>
static int for_each_sampler_batch(gat_ctx* ctx, gat_problem* P, const Knobs& kn, uint32_t seed, int64_t sample_begin, int64_t S,
                                  gat_stats& local, const BatchOpts& opts, After after_batch) {
  int rc;
  int64_t done = 0;
  while (done < S) {
    if ((rc = ensure_scratch(ctx, P, kn, S - done))) return rc;
    const int64_t nb = std::min<int64_t>(P->batch, S - done);
    if ((rc = run_sampler_batch(ctx, P, kn, seed, sample_begin + done, nb, &local, ctx->timed_owner == nullptr, opts)) == kRelayout) continue;
    if (rc) return rc;
    if ((rc = after_batch(done, nb))) return rc;
    local.n_batches += 1;
    done += nb;
  }
  return GAT_OK;
}

// the contig-level lists of a finished batch, as the kernels reach them (list_at)
static gat::ListSet sampled_lists(const gat_problem* P) {
  gat::ListSet S = {};
  S.seg = P->merge_contigs ? P->d_cslab.p : P->final_slab();
  S.seg_stride = P->slab_stride;
  S.c_off = P->d_count_c_off.p;
  S.n_arr = P->merge_contigs ? P->d_contig_n.p : P->d_unit_n.p;
  S.n_stride = P->merge_contigs ? P->n_contigs : P->n_units;
  S.n_index = P->d_count_n_index.p;
  return S;
}
// ... and whether they are normalized: SamplerSegments without isochore keys leaves them neither sorted nor disjoint
static bool sampled_lists_normalized(const gat_problem* P) { return !(P->sampler == GAT_SAMPLER_SEGMENTS && !P->merge_contigs); }

// offsets of n caller-provided lists of `noun`: GAT_ERR_ARG where they start below 0, decrease, or a list is longer than 2^31 - 1
static int check_list_offsets(gat_ctx* ctx, const char* who, const char* what, const char* noun, const int64_t* off, int64_t n) {
  if (off[0] < 0) return set_err(ctx, GAT_ERR_ARG, "%s: %s[0] < 0", who, what);
  for (int64_t l = 0; l < n; ++l)
    if (off[l + 1] < off[l] || off[l + 1] - off[l] > (int64_t)INT32_MAX)
      return set_err(ctx, GAT_ERR_ARG, "%s: %s decreases, or a list of more than 2^31 - 1 %s, at list %lld", who, what, noun, (long long)l);
  return GAT_OK;
}
// n caller-provided lists a[off[0] .. off[n]) on the device -- a call's segment lists, or the tracks it reads them against: the
// intervals built in the pinned staging buffer, the offsets from 0.  Like every device buffer of a call it is declared before
// the call's frame.
struct DevLists {
  DevBuf<uint2> d_seg;
  DevBuf<int64_t> d_csr;
  int upload(gat_ctx* ctx, const gat_segment* a, const int64_t* off, int64_t n) {
    const int64_t base = off[0], total = off[n] - base;
    HIPCHK(ctx, d_seg.upload_built((size_t)total, ctx, [&](uint2* h) {
      for (int64_t i = 0; i < total; ++i) h[i] = make_uint2(a[base + i].start, a[base + i].end);
    }));
    std::vector<int64_t> h_csr((size_t)n + 1);
    for (int64_t l = 0; l <= n; ++l) h_csr[(size_t)l] = off[l] - base;
    HIPCHK(ctx, d_csr.upload(h_csr, ctx));
    HIPCHK(ctx, stage_flush(ctx));                    // (h_csr goes away with this frame)
    return GAT_OK;
  }
  gat::ListSet view() const {
    gat::ListSet S = {};
    S.seg = d_seg.p;
    S.csr = d_csr.p;
    return S;
  }
};
// every one of n_entities x n_groups lists sorted, disjoint, without an empty interval; `why`: what the caller is told it is for
static int check_normalized(gat_ctx* ctx, const char* who, const char* what, const gat_segment* a, const int64_t* off,
                            int64_t n_entities, int32_t n_groups, const char* why) {
  for (int64_t i = 0; i < n_entities; ++i)
    for (int32_t g = 0; g < n_groups; ++g) {
      const int64_t b = off[i * n_groups + g], e = off[i * n_groups + g + 1];
      for (int64_t j = b; j < e; ++j)
        if (a[j].end <= a[j].start || (j > b && a[j].start < a[j - 1].end))
          return set_err(ctx, GAT_ERR_ARG, "%s: %s %lld, group %d is not normalized at interval %lld (sorted, disjoint, none empty: "
                         "%s)", who, what, (long long)i, g, (long long)(j - b), why);
    }
  return GAT_OK;
}
// what a call over n_lists x n_groups caller-provided lists asks of the two counts (before anything is indexed with them) ...
static int check_list_counts(gat_ctx* ctx, const char* who, int64_t n_lists, int32_t n_groups) {
  if (n_lists < 0 || n_groups < 0 || n_lists > (int64_t)INT32_MAX || n_lists * std::max<int64_t>(1, n_groups) > (int64_t)INT32_MAX)
    return set_err(ctx, GAT_ERR_ARG, "%s: n_lists %lld, n_groups %d", who, (long long)n_lists, n_groups);
  return GAT_OK;
}
// ... and of the lists themselves, once the other side of the call is checked; normalized where the call says why it needs that
static int check_caller_lists(gat_ctx* ctx, const char* who, const char* noun, const gat_segment* lists, const int64_t* list_off,
                              int64_t n_lists, int32_t n_groups, const char* why_normalized) {
  const int64_t n = n_lists * n_groups;
  const int rc = check_list_offsets(ctx, who, "list_off", noun, list_off, n);
  if (rc) return rc;
  if (list_off[n] > list_off[0] && !lists) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  return why_normalized ? check_normalized(ctx, who, "segment list", lists, list_off, n_lists, n_groups, why_normalized) : GAT_OK;
}
// what a call asks of the n_tracks x n_groups annotation tracks themselves, their number being in range (check_tracks, or a
// tool's own bound in its own words): the offsets, and the tracks normalized where the call says why it needs that
static int check_track_lists(gat_ctx* ctx, const char* who, const gat_segment* annos, const int64_t* anno_off, int64_t n_tracks, int64_t n_groups,
                             const char* why_normalized) {
  const int64_t n = n_tracks * n_groups;
  const int rc = check_list_offsets(ctx, who, "anno_off", "intervals", anno_off, n);
  if (rc) return rc;
  if (anno_off[n] > anno_off[0] && !annos) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  return why_normalized ? check_normalized(ctx, who, "annotation track", annos, anno_off, n_tracks, (int32_t)n_groups, why_normalized) : GAT_OK;
}
// ... and of their number, where 32-bit indices are the only bound on it
static int check_tracks(gat_ctx* ctx, const char* who, const gat_segment* annos, const int64_t* anno_off, int64_t n_tracks, int64_t n_groups,
                        const char* why_normalized) {
  if (n_tracks < 0 || n_tracks > (int64_t)INT32_MAX || n_tracks * std::max<int64_t>(1, n_groups) > (int64_t)INT32_MAX)
    return set_err(ctx, GAT_ERR_ARG, "%s: n_tracks %lld", who, (long long)n_tracks);
  return check_track_lists(ctx, who, annos, anno_off, n_tracks, n_groups, why_normalized);
}
// bins of bin_size bases, bin_off[0 .. n] of them per `unit` (the caller's word: contig, group)
static int check_bins(gat_ctx* ctx, const char* who, int64_t bin_size, const int64_t* bin_off, int64_t n, const char* unit) {
  if (bin_size < 1 || bin_size > (int64_t)1 << 31) return set_err(ctx, GAT_ERR_ARG, "%s: bin_size %lld outside [1, 2^31]", who, (long long)bin_size);
  if (bin_off[0] < 0) return set_err(ctx, GAT_ERR_ARG, "%s: bin_off[0] < 0", who);
  for (int64_t c = 0; c < n; ++c)
    if (bin_off[c + 1] < bin_off[c]) return set_err(ctx, GAT_ERR_ARG, "%s: bin_off decreases at %s %lld", who, unit, (long long)c);
  return GAT_OK;
}
static int check_sample_range(gat_ctx* ctx, int64_t sample_begin, int64_t sample_end) {
  return sample_end < sample_begin ? set_err(ctx, GAT_ERR_ARG, "sample_end < sample_begin") : GAT_OK;
}
// a reduction that needs the sampled lists normalized refuses a problem whose lists are not; `needs`: who needs it, in the caller's words
static int check_sampled_lists_normalized(gat_ctx* ctx, const char* who, const gat_problem* P, const char* needs) {
  if (sampled_lists_normalized(P)) return GAT_OK;
  return set_err(ctx, GAT_ERR_ARG, "%s: the sampled segment lists are not normalized (SamplerSegments without isochore keys leaves them "
                 "neither sorted nor disjoint): %s", who, needs);
}
// k_store (the raw values per list) or k_fold (the fold into the five words), with `lds` bytes of dynamic LDS
template <class Args>
static int launch_store_or_fold(gat_ctx* ctx, bool store, void (*k_store)(Args), void (*k_fold)(Args), dim3 grid, int threads, size_t lds, const Args& A) {
  void (*const k)(Args) = store ? k_store : k_fold;
  HIPCHK(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, grid, dim3(threads), lds, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  return GAT_OK;
}

// ---- the fold of the sampled null to five words per cell (gat_null_words.h), as gat_sample_bin_enrichment,
// gat_sample_pair_enrichment, gat_sample_geneset_enrichment, gat_sample_profile_enrichment, gat_sample_reldist_enrichment and gat_sample_metagene_enrichment share it: obs up and the words zeroed before the first batch,
// k_null_finish and the words down behind the last
struct NullWordsOut {
  DevBuf<long long> d_obs;
  DevBuf<unsigned long long> d_out;         // (the calls over caller-provided lists keep their raw values here)
  int begin(gat_ctx* ctx, const int64_t* obs_host, int64_t n) {
    HIPCHK(ctx, d_obs.alloc((size_t)n));
    HIPCHK(ctx, staged_h2d(ctx, d_obs.p, obs_host, (size_t)n * 8));
    HIPCHK(ctx, d_out.alloc((size_t)n * gat::kNullWords));
    HIPCHK(ctx, hipMemsetAsync(d_out.p, 0, (size_t)n * gat::kNullWords * 8, ctx->stream));
    return GAT_OK;
  }
  int finish(gat_ctx* ctx, int64_t n, int64_t S, int64_t* out_host) {
    hipLaunchKernelGGL(gat::k_null_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_out.p, d_obs.p, n, (unsigned long long)S);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, staged_d2h(ctx, out_host, d_out.p, (size_t)n * gat::kNullWords * 8));
    return GAT_OK;
  }
};
// what the three ask of the range and of obs: a value is at most `bound` (`bound_name` and `advice`: the caller's words for
// it), so sumsq <= bound^2 * S has to fit 64 bits; obs[0 .. n) >= 0
static int check_null_words(gat_ctx* ctx, const char* who, const char* bound_name, int64_t bound, const char* advice, int64_t S,
                            const int64_t* obs_host, int64_t n) {
  if ((unsigned __int128)((uint64_t)bound * (uint64_t)bound) * (unsigned __int128)(uint64_t)S >> 64)
    return set_err(ctx, GAT_ERR_ARG, "%s: %s^2 * samples = %lld^2 * %lld does not fit 64 bits (sumsq): %s", who, bound_name,
                   (long long)bound, (long long)S, advice);
  for (int64_t k = 0; k < n; ++k)
    if (obs_host[k] < 0) return set_err(ctx, GAT_ERR_ARG, "%s: obs[%lld] = %lld is negative", who, (long long)k, (long long)obs_host[k]);
  return GAT_OK;
}

// ---- the two calls of a tool that reduces lists against something of its own (tracks, genes, anchors).  The tool is a struct
// T of what the caller gave and the device buffers made from it -- declared by the entry point, which has checked the
// arguments, BEFORE the call, so destroyed after its frame -- with
//   T.upload(ctx, kn, n_groups, n_lists)                   the tool's side onto the device, for a call over n_lists lists in all
//   T.launch(ctx, kn, lists, n_lists, n_groups, store)     one launch over n_lists lists: the raw values per list into T.out.d_out
//                                                          (store), or their fold into T.out's five words

// The raw values of the caller's n_lists x n_groups lists, words_per_list each, from T.out.d_out (zeroed here) to out_host.
// Nothing to write: nothing is done.
template <class Tool>
static int store_over_caller_lists(gat_ctx* ctx, Tool& T, const gat_segment* lists, const int64_t* list_off,
                                   int64_t n_lists, int32_t n_groups, int64_t words_per_list, int64_t* out_host) {
  const size_t words = (size_t)(n_lists * words_per_list);
  if (words == 0) return GAT_OK;
  DevLists L;
  DevBuf<unsigned long long>& d_out = T.out.d_out;
  return call_frame(ctx, nullptr, nullptr, [&](const Knobs& kn, gat_stats&) {
    int rc;
    if ((rc = T.upload(ctx, kn, n_groups, n_lists))) return rc;
    if ((rc = L.upload(ctx, lists, list_off, n_lists * n_groups))) return rc;
    HIPCHK(ctx, d_out.alloc(words));
    HIPCHK(ctx, hipMemsetAsync(d_out.p, 0, words * 8, ctx->stream));
    if ((rc = T.launch(ctx, kn, L.view(), n_lists, n_groups, true))) return rc;
    HIPCHK(ctx, staged_d2h(ctx, out_host, d_out.p, words * 8));
    return GAT_OK;
  });
}
// The fold of the sampled null of `cells` cells over S samples, a launch behind every batch.  No cell -- nothing is written; no
// sample -- no batch runs, the sums are empty.
template <class Tool>
static int fold_over_sampled_batches(gat_ctx* ctx, gat_problem* P, gat_stats* stats, uint32_t seed, int64_t sample_begin, int64_t S, Tool& T,
                                     const int64_t* obs_host, int64_t cells, int64_t* out_host) {
  return call_frame(ctx, P, stats, [&](const Knobs& kn, gat_stats& local) {
    if (cells == 0) return GAT_OK;
    if (S == 0) { memset(out_host, 0, (size_t)cells * gat::kNullWords * 8); return GAT_OK; }
    const int C = P->n_contigs;
    int rc;
    if ((rc = T.upload(ctx, kn, C, S))) return rc;
    if ((rc = T.out.begin(ctx, obs_host, cells))) return rc;
    rc = for_each_sampler_batch(ctx, P, kn, seed, sample_begin, S, local, BatchOpts(), [&](int64_t, int64_t nb) {
      return T.launch(ctx, kn, sampled_lists(P), nb, C, false);
    });
    return rc ? rc : T.out.finish(ctx, cells, S, out_host);
  });
}

// gat_sample / gat_sample_units: the lists of every (sample, contig) after fromIsochores, or of every (sample, unit)
// as the sampler returned them
static int sample_lists_body(gat_ctx* ctx, gat_problem* P, const Knobs& kn, uint32_t seed, int64_t sample_begin, int64_t S,
                             gat_segment* out_host, int64_t cap, int64_t* off_host, gat_stats& local, bool unit_level) {
  const int C = unit_level ? P->n_units : P->n_contigs;
  int64_t total = 0;
  bool overflow = false;
  off_host[0] = 0;
  std::vector<uint2> h_slab;
  std::vector<int32_t> h_n;
  BatchOpts o;
  o.need_unit_lists = unit_level;
  const int rc = for_each_sampler_batch(ctx, P, kn, seed, sample_begin, S, local, o, [&](int64_t done, int64_t nb) {
    const bool from_contigs = P->merge_contigs && !unit_level;
    const uint2* src = from_contigs ? P->d_cslab.p : P->final_slab();
    const int32_t* nsrc = from_contigs ? P->d_contig_n.p : P->d_unit_n.p;
    const int nstride = from_contigs ? P->n_contigs : P->n_units;
    h_slab.resize((size_t)(nb * P->slab_stride));
    h_n.resize((size_t)(nb * std::max(1, nstride)));
    HIPCHK(ctx, staged_d2h(ctx, h_slab.data(), src, h_slab.size() * sizeof(uint2)));
    HIPCHK(ctx, staged_d2h(ctx, h_n.data(), nsrc, h_n.size() * 4));
    for (int64_t i = 0; i < nb; ++i) {
      for (int c = 0; c < C; ++c) {
        // (units that computeSample skips keep n == 0: their entries are never written and were zeroed at allocation)
        const int32_t n = unit_level ? h_n[(size_t)(i * nstride + c)] : h_n[(size_t)(i * nstride + P->h_count_n_index[c])];
        const int64_t soff = unit_level ? (int64_t)P->h_units[(size_t)c].slab_off : (int64_t)P->h_count_c_off[c];
        if (!overflow && out_host && total + n <= cap)
          memcpy(out_host + total, h_slab.data() + i * P->slab_stride + soff, (size_t)n * sizeof(uint2));
        else if (n > 0) overflow = true;
        total += n;
        off_host[(done + i) * C + c + 1] = total;
      }
    }
    return GAT_OK;
  });
  if (rc) return rc;
  local.n_sampled_segments = total;
  if (overflow) return set_err(ctx, GAT_ERR_CAPACITY, "gat_sample: output needs %lld segments, cap is %lld", (long long)total, (long long)cap);
  return GAT_OK;
}
static int sample_lists(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                        gat_segment* out_host, int64_t cap, int64_t* off_host, gat_stats* stats, bool unit_level) {
  if (!ctx || !P || !off_host) return set_err(ctx, GAT_ERR_ARG, "gat_sample: NULL argument");
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  return call_frame(ctx, P, stats, [&](const Knobs& kn, gat_stats& local) {
    return sample_lists_body(ctx, P, kn, seed, sample_begin, sample_end - sample_begin, out_host, cap, off_host, local, unit_level);
  });
}

extern "C" int gat_sample(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                          gat_segment* out_host, int64_t cap, int64_t* off_host, gat_stats* stats) {
  return sample_lists(ctx, P, seed, sample_begin, sample_end, out_host, cap, off_host, stats, false);
}
extern "C" int gat_sample_units(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                gat_segment* out_host, int64_t cap, int64_t* off_host, gat_stats* stats) {
  return sample_lists(ctx, P, seed, sample_begin, sample_end, out_host, cap, off_host, stats, true);
}

// gat_sample_coverage: k_coverage (gat_coverage.h) behind every batch, where sample_lists copies the lists out.  The device
// result lives for the call.
struct CoverageBufs {
  DevBuf<gat::CoverageWindow> d_win;
  DevBuf<unsigned long long> d_bases, d_starts, d_ends, d_outside;
};
static int sample_coverage_body(gat_ctx* ctx, gat_problem* P, const Knobs& kn, uint32_t seed, int64_t sample_begin, int64_t S,
                                int64_t bin_size, const int64_t* bin_off, int64_t* bases_host, int64_t* starts_host,
                                int64_t* ends_host, int64_t* outside_host, gat_stats& local, CoverageBufs& B) {
  const int C = P->n_contigs;
  const int64_t total = bin_off[C];
  const bool want_se = starts_host != nullptr || ends_host != nullptr;
  // the windows: W bins each, then the contig's tail.  Coordinates are below 2^32: bins beyond that stay 0 and get no window
  const int64_t W = std::max<int64_t>(1, std::min<int64_t>(kn.coverage_window_bins, ((int64_t)ctx->max_lds - 1024) / gat::kCoverageBinBytes));
  const int64_t reach = (((int64_t)1 << 32) + bin_size - 1) / bin_size;
  std::vector<gat::CoverageWindow> win;
  for (int c = 0; c < C; ++c) {
    const int64_t n_bins = bin_off[c + 1] - bin_off[c], eff = std::min(n_bins, reach);
    for (int64_t b = 0; b < eff; b += W) win.push_back({b * bin_size, bin_off[c] + b, c, (int32_t)std::min(W, eff - b)});
    win.push_back({n_bins < reach ? n_bins * bin_size : (int64_t)1 << 32, 0, c, 0});
    if (win.size() >= (size_t)INT32_MAX) return set_err(ctx, GAT_ERR_CAPACITY, "gat_sample_coverage: more than 2^31 windows of %lld bins", (long long)W);
  }
  HIPCHK(ctx, B.d_win.upload(win, ctx));
  HIPCHK(ctx, B.d_bases.alloc((size_t)total));
  HIPCHK(ctx, B.d_outside.alloc((size_t)C));
  HIPCHK(ctx, hipMemsetAsync(B.d_bases.p, 0, B.d_bases.bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(B.d_outside.p, 0, B.d_outside.bytes, ctx->stream));
  if (want_se) {
    HIPCHK(ctx, B.d_starts.alloc((size_t)total));
    HIPCHK(ctx, B.d_ends.alloc((size_t)total));
    HIPCHK(ctx, hipMemsetAsync(B.d_starts.p, 0, B.d_starts.bytes, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(B.d_ends.p, 0, B.d_ends.bytes, ctx->stream));
  }
  const size_t lds = gat::coverage_lds_bytes(W);
  HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_coverage, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int rc = for_each_sampler_batch(ctx, P, kn, seed, sample_begin, S, local, BatchOpts(), [&](int64_t, int64_t nb) {
    if (win.empty()) return GAT_OK;
    gat::CoverageArgs A;
    A.lists = sampled_lists(P);
    A.n_samples = (int32_t)nb;
    A.window_bins = (int32_t)W;
    A.sorted = sampled_lists_normalized(P) ? 1 : 0;
    A.bin_size = bin_size;
    A.win = B.d_win.p;
    A.bases = B.d_bases.p; A.starts = want_se ? B.d_starts.p : nullptr; A.ends = want_se ? B.d_ends.p : nullptr; A.outside = B.d_outside.p;
    const int64_t spb = gat::coverage_run_per_block(nb, (int64_t)win.size(), kn.coverage_samples_per_block, P->slab_stride);
    A.samples_per_block = (int32_t)spb;
    hipLaunchKernelGGL(gat::k_coverage, dim3((unsigned)win.size(), (unsigned)((nb + spb - 1) / spb)), dim3(gat::kCoverageThreads), lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return GAT_OK;
  });
  if (rc) return rc;
  if (total > 0) HIPCHK(ctx, staged_d2h(ctx, bases_host, B.d_bases.p, (size_t)total * 8));
  if (total > 0 && starts_host) HIPCHK(ctx, staged_d2h(ctx, starts_host, B.d_starts.p, (size_t)total * 8));
  if (total > 0 && ends_host) HIPCHK(ctx, staged_d2h(ctx, ends_host, B.d_ends.p, (size_t)total * 8));
  if (C > 0) HIPCHK(ctx, staged_d2h(ctx, outside_host, B.d_outside.p, (size_t)C * 8));
  return GAT_OK;
}

extern "C" int gat_sample_coverage(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                   int64_t bin_size, const int64_t* bin_off, int64_t* bases_host, int64_t* starts_host,
                                   int64_t* ends_host, int64_t* outside_host, gat_stats* stats) {
  if (!ctx || !P || !bin_off || !bases_host || !outside_host) return set_err(ctx, GAT_ERR_ARG, "gat_sample_coverage: NULL argument");
  if (int rc = check_bins(ctx, "gat_sample_coverage", bin_size, bin_off, P->n_contigs, "contig")) return rc;
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  CoverageBufs B;
  return call_frame(ctx, P, stats, [&](const Knobs& kn, gat_stats& local) {
    const int64_t total = bin_off[P->n_contigs], S = sample_end - sample_begin;
    if (S == 0) {                                                  // (no batch runs: the sums are empty)
      memset(bases_host, 0, (size_t)total * 8);
      if (starts_host) memset(starts_host, 0, (size_t)total * 8);
      if (ends_host) memset(ends_host, 0, (size_t)total * 8);
      memset(outside_host, 0, (size_t)P->n_contigs * 8);
      return GAT_OK;
    }
    return sample_coverage_body(ctx, P, kn, seed, sample_begin, S, bin_size, bin_off, bases_host, starts_host, ends_host,
                                outside_host, local, B);
  });
}

// gat_list_metrics / gat_sample_metrics: k_metrics (gat_metrics.h) over caller-provided lists, or behind every batch.  The
// groups' pieces and their prefix tables (gat_metrics_tables.h) are made on the host per call.  The device buffers live for
// the call.
struct MetricsBufs {
  DevBuf<uint32_t> d_start, d_end, d_gaps;
  DevBuf<unsigned long long> d_cum;
  DevBuf<int32_t> d_off;
  DevLists lists;
  DevBuf<long long> d_out;
};
static int metrics_upload_groups(gat_ctx* ctx, const gat_segment* ws, const int64_t* ws_off, int64_t n_groups, MetricsBufs& B, const char* who) {
  MetricsTables T;
  std::string err;
  const int rc = metrics_build_tables(ws, ws_off, n_groups, T, err);
  if (rc) return set_err(ctx, rc, "%s: %s", who, err.c_str());
  HIPCHK(ctx, B.d_start.upload(T.start, ctx));
  HIPCHK(ctx, B.d_end.upload(T.end, ctx));
  HIPCHK(ctx, B.d_gaps.upload(T.gaps, ctx));
  HIPCHK(ctx, B.d_cum.upload(T.cum, ctx));
  HIPCHK(ctx, B.d_off.upload(T.off, ctx));
  HIPCHK(ctx, stage_flush(ctx));                    // (T goes away with this frame: the pushed copies have read it, but be plain about it)
  return GAT_OK;
}
// the launch over n_lists x A.n_groups lists: a wave per list, a workgroup per group and run of lists -- the run as long as
// leaves 2 048 workgroups (eight for each of 256 compute units) but at least 16 lists, so that staging a group's pieces is
// shared by many lists; within the grid's y
static int launch_metrics(gat_ctx* ctx, const Knobs& kn, gat::MetricsArgs A, int64_t n_lists, const MetricsBufs& B) {
  if (n_lists == 0 || A.n_groups == 0) return GAT_OK;
  const int64_t L = std::max<int64_t>(1, std::min<int64_t>(kn.metrics_lds_pieces, ((int64_t)ctx->max_lds - 1024) / 8));
  const int64_t lpb = gat::run_per_block(n_lists, A.n_groups, 2048, gat::kNoRunCap);
  A.n_lists = (int32_t)n_lists;
  A.lists_per_block = (int32_t)lpb;
  A.lds_pieces = (int32_t)L;
  A.ws_start = B.d_start.p; A.ws_end = B.d_end.p; A.ws_cum = B.d_cum.p; A.ws_gaps = B.d_gaps.p; A.ws_off = B.d_off.p;
  A.out = B.d_out.p;
  const size_t lds = gat::metrics_lds_bytes(L);
  HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_metrics, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(gat::k_metrics, dim3((unsigned)A.n_groups, (unsigned)((n_lists + lpb - 1) / lpb)), dim3(gat::kMetricsThreads), lds, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  return GAT_OK;
}

static int list_metrics_body(gat_ctx* ctx, const Knobs& kn, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                             const gat_segment* ws, const int64_t* ws_off, int32_t n_groups, int64_t* out_host, MetricsBufs& B) {
  const int64_t n = n_lists * n_groups;
  int rc;
  if (n == 0) {                                     // (no list: only the groups are looked at)
    MetricsTables T;
    std::string err;
    rc = metrics_build_tables(ws, ws_off, n_groups, T, err);
    return rc ? set_err(ctx, rc, "gat_list_metrics: %s", err.c_str()) : GAT_OK;
  }
  if ((rc = metrics_upload_groups(ctx, ws, ws_off, n_groups, B, "gat_list_metrics"))) return rc;
  if ((rc = B.lists.upload(ctx, lists, list_off, n))) return rc;
  HIPCHK(ctx, B.d_out.alloc((size_t)n * gat::kMetricsWords));
  gat::MetricsArgs A;
  memset(&A, 0, sizeof(A));
  A.lists = B.lists.view();
  A.n_groups = n_groups;
  if ((rc = launch_metrics(ctx, kn, A, n_lists, B))) return rc;
  HIPCHK(ctx, staged_d2h(ctx, out_host, B.d_out.p, (size_t)n * gat::kMetricsWords * 8));
  return GAT_OK;
}

extern "C" int gat_list_metrics(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                const gat_segment* ws, const int64_t* ws_off, int32_t n_groups, int64_t* out_host) {
  if (!ctx || !list_off || !ws_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "gat_list_metrics: NULL argument");
  if (n_lists < 0 || n_groups < 0 || n_lists > (int64_t)INT32_MAX) return set_err(ctx, GAT_ERR_ARG, "gat_list_metrics: n_lists %lld, n_groups %d", (long long)n_lists, n_groups);
  const int64_t n = n_lists * n_groups;
  int rc;
  if ((rc = check_list_offsets(ctx, "gat_list_metrics", "list_off", "segments", list_off, n))) return rc;
  if (list_off[n] > list_off[0] && !lists) return set_err(ctx, GAT_ERR_ARG, "gat_list_metrics: NULL argument");
  for (int64_t i = list_off[0]; i < list_off[n]; ++i)
    if (lists[i].end < lists[i].start) return set_err(ctx, GAT_ERR_ARG, "gat_list_metrics: segment %lld ends before it starts", (long long)i);
  MetricsBufs B;
  return call_frame(ctx, nullptr, nullptr, [&](const Knobs& kn, gat_stats&) {
    return list_metrics_body(ctx, kn, lists, list_off, n_lists, ws, ws_off, n_groups, out_host, B);
  });
}

static int sample_metrics_body(gat_ctx* ctx, gat_problem* P, const Knobs& kn, uint32_t seed, int64_t sample_begin, int64_t S,
                               const gat_segment* ws, const int64_t* ws_off, int64_t* out_host, gat_stats& local, MetricsBufs& B) {
  const int C = P->n_contigs;
  int rc;
  if ((rc = metrics_upload_groups(ctx, ws, ws_off, C, B, "gat_sample_metrics"))) return rc;
  return for_each_sampler_batch(ctx, P, kn, seed, sample_begin, S, local, BatchOpts(), [&](int64_t done, int64_t nb) {
    if (C == 0) return GAT_OK;
    if (B.d_out.n < (size_t)(nb * C * gat::kMetricsWords)) HIPCHK(ctx, B.d_out.alloc((size_t)(nb * C * gat::kMetricsWords)));
    gat::MetricsArgs A;
    memset(&A, 0, sizeof(A));
    A.lists = sampled_lists(P);
    A.n_groups = C;
    const int lrc = launch_metrics(ctx, kn, A, nb, B);
    if (lrc) return lrc;
    HIPCHK(ctx, staged_d2h(ctx, out_host + done * C * gat::kMetricsWords, B.d_out.p, (size_t)(nb * C * gat::kMetricsWords) * 8));
    return GAT_OK;
  });
}

extern "C" int gat_sample_metrics(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                  const gat_segment* ws, const int64_t* ws_off, int64_t* out_host, gat_stats* stats) {
  if (!ctx || !P || !ws_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "gat_sample_metrics: NULL argument");
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  MetricsBufs B;
  return call_frame(ctx, P, stats, [&](const Knobs& kn, gat_stats& local) {
    return sample_metrics_body(ctx, P, kn, seed, sample_begin, sample_end - sample_begin, ws, ws_off, out_host, local, B);
  });
}

// gat_list_distances / gat_sample_distances: k_distance (gat_distance.h) over caller-provided lists, or behind every batch.
// The annotation tracks go up once per call as they are given (CSR, uint2); the device buffers live for the call.
static const char* const kDistanceWhy = "the nearest interval is searched for in it";
struct DistanceCall {
  const char* who;
  const gat_segment* annos; const int64_t* anno_off; int32_t n_tracks; int direction; int64_t max_distance;
  DevLists tracks;
  struct { DevBuf<unsigned long long> d_out; } out;      // (T.out.d_out, as in the tools that fold: the store frame fills it)
  // what both entry points ask of the direction, the bound and the tracks: the searched side in direction 0
  int check(gat_ctx* ctx, int64_t n_groups) const {
    if (direction != GAT_DISTANCE_SEGMENT_TO_ANNOTATION && direction != GAT_DISTANCE_ANNOTATION_TO_SEGMENT)
      return set_err(ctx, GAT_ERR_ARG, "%s: direction %d is neither GAT_DISTANCE_SEGMENT_TO_ANNOTATION nor GAT_DISTANCE_ANNOTATION_TO_SEGMENT", who, direction);
    if (max_distance < 0 || max_distance > (int64_t)1 << 32) return set_err(ctx, GAT_ERR_ARG, "%s: max_distance %lld outside [0, 2^32]", who, (long long)max_distance);
    return check_tracks(ctx, who, annos, anno_off, n_tracks, n_groups,
                        direction == GAT_DISTANCE_SEGMENT_TO_ANNOTATION ? kDistanceWhy : nullptr);
  }
  int upload(gat_ctx* ctx, const Knobs&, int32_t n_groups, int64_t) { return tracks.upload(ctx, annos, anno_off, (int64_t)n_tracks * n_groups); }
  // the launch over n_lists x n_tracks x n_groups pairs of lists, `lists` in either layout.  A workgroup stages one list of the
  // searched side -- the tracks' in direction 0, the segment lists' in direction 1 -- and takes a run of the other side's: the
  // run as long as leaves 2 048 workgroups (eight for each of 256 compute units) but at least 16 lists, within the grid's y.
  // out.d_out holds n_lists * n_tracks * 4 words, zeroed by the caller: the kernel only ever stores (the flag says nothing here).
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool) const {
    if (n_lists == 0 || n_tracks == 0 || n_groups == 0) return GAT_OK;
    gat::DistanceArgs A;
    memset(&A, 0, sizeof(A));
    const bool seg_to_anno = direction == GAT_DISTANCE_SEGMENT_TO_ANNOTATION;
    A.t = seg_to_anno ? tracks.view() : lists;
    A.q = seg_to_anno ? lists : tracks.view();
    const int64_t n_t = seg_to_anno ? n_tracks : n_lists, n_q = seg_to_anno ? n_lists : n_tracks;
    if (n_t * n_groups > (int64_t)INT32_MAX) return set_err(ctx, GAT_ERR_CAPACITY, "gat distances: %lld x %d searched lists in one launch", (long long)n_t, n_groups);
    A.n_t = (int32_t)n_t;
    A.n_q = (int32_t)n_q;
    A.n_groups = n_groups;
    A.out_stride_t = seg_to_anno ? 1 : n_tracks;
    A.out_stride_q = seg_to_anno ? n_tracks : 1;
    A.max_distance = (unsigned long long)max_distance;
    A.out = out.d_out.p;
    const int64_t L = std::max<int64_t>(1, std::min<int64_t>(kn.distance_lds_pieces, ((int64_t)ctx->max_lds - 1024) / 8));
    A.lds_pieces = (int32_t)L;
    const int64_t qpb = gat::run_per_block(n_q, n_t * n_groups, 2048, gat::kNoRunCap);
    A.q_per_block = (int32_t)qpb;
    const size_t lds = gat::distance_lds_bytes(L);
    HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_distance, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gat::k_distance, dim3((unsigned)(n_t * n_groups), (unsigned)((n_q + qpb - 1) / qpb)), dim3(gat::kDistanceThreads), lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return GAT_OK;
  }
};

extern "C" int gat_list_distances(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                  const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int32_t n_groups,
                                  int direction, int64_t max_distance, int64_t* out_host) {
  const char* who = "gat_list_distances";
  if (!ctx || !list_off || !anno_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  DistanceCall T = {who, annos, anno_off, n_tracks, direction, max_distance};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = check_caller_lists(ctx, who, "intervals", lists, list_off, n_lists, n_groups,
                               direction == GAT_DISTANCE_ANNOTATION_TO_SEGMENT ? kDistanceWhy : nullptr))) return rc;
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, (int64_t)n_tracks * gat::kDistanceWords, out_host);
}

// (not the fold: the words of a batch are copied out behind it, and an empty range writes nothing)
extern "C" int gat_sample_distances(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                    const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int direction,
                                    int64_t max_distance, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_distances";
  if (!ctx || !P || !anno_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  DistanceCall T = {who, annos, anno_off, n_tracks, direction, max_distance};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  // the searched side of direction 1 is the sampler's: the flag k_coverage gets
  if (direction == GAT_DISTANCE_ANNOTATION_TO_SEGMENT &&
      (rc = check_sampled_lists_normalized(ctx, who, P, "GAT_DISTANCE_ANNOTATION_TO_SEGMENT searches them and needs normalized lists"))) return rc;
  return call_frame(ctx, P, stats, [&](const Knobs& kn, gat_stats& local) {
    const int C = P->n_contigs;
    const int64_t S = sample_end - sample_begin;
    if (S == 0) return GAT_OK;                        // (no batch runs: nothing is written)
    const int urc = T.upload(ctx, kn, C, S);
    if (urc) return urc;
    return for_each_sampler_batch(ctx, P, kn, seed, sample_begin, S, local, BatchOpts(), [&](int64_t done, int64_t nb) {
      const size_t words = (size_t)(nb * n_tracks * gat::kDistanceWords);
      if (words == 0) return GAT_OK;
      if (T.out.d_out.n < words) HIPCHK(ctx, T.out.d_out.alloc(words));
      HIPCHK(ctx, hipMemsetAsync(T.out.d_out.p, 0, words * 8, ctx->stream));
      const int lrc = T.launch(ctx, kn, sampled_lists(P), nb, C, true);
      if (lrc) return lrc;
      HIPCHK(ctx, staged_d2h(ctx, out_host + done * n_tracks * gat::kDistanceWords, T.out.d_out.p, words * 8));
      return GAT_OK;
    });
  });
}

// gat_list_signal / gat_sample_signal: k_signal (gat_signal.h) over caller-provided lists, or behind every batch.  The signal
// tracks go up once per call as 32-byte records -- piece, value and the two prefix sums before it (gat_signal_sum.h) -- built
// in upload; the device buffers live for the call.
static const char* const kSignalWhy = "the pieces are searched and their prefix sums are formed over it";
struct SignalCall {
  const char* who;
  const gat_segment* pieces; const int32_t* values; const int64_t* piece_off; int32_t n_tracks;
  DevBuf<gat::SignalPiece> d_rec;
  DevBuf<int64_t> d_off;
  struct { DevBuf<unsigned long long> d_out; } out;      // (T.out.d_out: the store frame fills it)
  std::vector<unsigned __int128> M;                      // [track][group]: sum_k |q_k| * (e_k - s_k)
  // what both entry points ask of the tracks: normalized, no value of INT32_MIN, and sum_g M[t][g] < 2^63 -- the bound of
  // normalized segment lists, and the least any list asks
  int check(gat_ctx* ctx, int64_t n_groups) {
    int rc;
    if ((rc = check_tracks(ctx, who, pieces, piece_off, n_tracks, n_groups, kSignalWhy))) return rc;
    const int64_t n = (int64_t)n_tracks * n_groups;
    if (piece_off[n] > piece_off[0] && !values) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    M.assign((size_t)n, 0);
    for (int64_t t = 0; t < n_tracks; ++t) {
      unsigned __int128 total = 0;
      for (int64_t g = 0; g < n_groups; ++g) {
        unsigned __int128 m = 0;
        for (int64_t k = piece_off[t * n_groups + g]; k < piece_off[t * n_groups + g + 1]; ++k) {
          if (values[k] == INT32_MIN)
            return set_err(ctx, GAT_ERR_ARG, "%s: signal track %lld, group %lld: the value of piece %lld is INT32_MIN (|q| <= 2^31 - 1)", who,
                           (long long)t, (long long)g, (long long)(k - piece_off[t * n_groups + g]));
          m += (unsigned __int128)(uint64_t)std::llabs((long long)values[k]) * (uint64_t)(pieces[k].end - pieces[k].start);
        }
        M[(size_t)(t * n_groups + g)] = m;
        total += m;
      }
      if (total >> 63) return refuse_bound(ctx, t, "the sum over its groups of |value| * length", nullptr);
    }
    return GAT_OK;
  }
  int refuse_bound(gat_ctx* ctx, int64_t t, const char* what, const char* advice) const {
    return set_err(ctx, GAT_ERR_ARG, "%s: signal track %lld: %s reaches 2^63: a sum could leave 64 bits%s%s", who, (long long)t, what,
                   advice ? ": " : "", advice ? advice : "");
  }
  // ... and of segment lists that are not normalized, n_g[g] of them at most on group g: a base counts once per segment that
  // covers it, so sum_g n_g * M[t][g] < 2^63.  (M[t][g] < 2^63 and n_g < 2^31 after check: the products and their sum fit 128 bits)
  int check_any_lists(gat_ctx* ctx, const int64_t* n_g, int64_t n_groups, const char* advice) const {
    for (int64_t t = 0; t < n_tracks; ++t) {
      unsigned __int128 total = 0;
      for (int64_t g = 0; g < n_groups; ++g) total += (unsigned __int128)(uint64_t)n_g[g] * M[(size_t)(t * n_groups + g)];
      if (total >> 63) return refuse_bound(ctx, t, "the sum over its groups of segments * |value| * length, for segment lists that are not normalized,", advice);
    }
    return GAT_OK;
  }
  int upload(gat_ctx* ctx, const Knobs&, int32_t n_groups, int64_t) {
    const int64_t n = (int64_t)n_tracks * n_groups, base = piece_off[0], total = piece_off[n] - base;
    HIPCHK(ctx, d_rec.upload_built((size_t)total, ctx, [&](gat::SignalPiece* h) {
      for (int64_t i = 0; i < n; ++i) {
        const int64_t b = piece_off[i];
        gat::signal_fill(h + (b - base), piece_off[i + 1] - b, [&](int64_t k, uint32_t& s, uint32_t& e, int32_t& q) {
          s = pieces[b + k].start; e = pieces[b + k].end; q = values[b + k];
        });
      }
    }));
    std::vector<int64_t> h_off((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) h_off[(size_t)i] = piece_off[i] - base;
    HIPCHK(ctx, d_off.upload(h_off, ctx));
    HIPCHK(ctx, stage_flush(ctx));                    // (h_off goes away with this frame)
    return GAT_OK;
  }
  // the launch over n_lists x n_tracks x n_groups: a workgroup stages the ends of one (track, group) and takes a run of the
  // lists: the run as long as leaves 2 048 workgroups (eight for each of 256 compute units) but at least 16 lists, within the
  // grid's y.  out.d_out holds n_lists * n_tracks * 4 words, zeroed by the caller (the flag says nothing here).
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool) const {
    if (n_lists == 0 || n_tracks == 0 || n_groups == 0) return GAT_OK;
    gat::SignalArgs A;
    memset(&A, 0, sizeof(A));
    A.q = lists;
    A.rec = d_rec.p;
    A.rec_off = d_off.p;
    A.n_tracks = n_tracks;
    A.n_q = (int32_t)n_lists;
    A.n_groups = n_groups;
    A.out = out.d_out.p;
    const int64_t L = std::max<int64_t>(1, std::min<int64_t>(kn.signal_lds_pieces, ((int64_t)ctx->max_lds - 1024) / 4));
    A.lds_pieces = (int32_t)L;
    const int64_t qpb = gat::run_per_block(n_lists, (int64_t)n_tracks * n_groups, 2048, gat::kNoRunCap);
    A.q_per_block = (int32_t)qpb;
    const size_t lds = gat::signal_lds_bytes(L);
    HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_signal, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gat::k_signal, dim3((unsigned)((int64_t)n_tracks * n_groups), (unsigned)((n_lists + qpb - 1) / qpb)), dim3(gat::kSignalThreads), lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return GAT_OK;
  }
};

extern "C" int gat_list_signal(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                               const gat_segment* pieces, const int32_t* values, const int64_t* piece_off,
                               int32_t n_tracks, int32_t n_groups, int64_t* out_host) {
  const char* who = "gat_list_signal";
  if (!ctx || !list_off || !piece_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  SignalCall T = {who, pieces, values, piece_off, n_tracks};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = check_caller_lists(ctx, who, "segments", lists, list_off, n_lists, n_groups, nullptr))) return rc;
  // the lists the host does not find normalized: the most segments one of them has on each group
  std::vector<int64_t> n_g((size_t)n_groups, 0);
  bool any = false;
  for (int64_t l = 0; l < n_lists; ++l) {
    bool normalized = true;
    for (int64_t j = list_off[l * n_groups]; j < list_off[(l + 1) * n_groups] && normalized; ++j)
      normalized = lists[j].end > lists[j].start;
    for (int32_t g = 0; g < n_groups && normalized; ++g)
      for (int64_t j = list_off[l * n_groups + g] + 1; j < list_off[l * n_groups + g + 1] && normalized; ++j)
        normalized = lists[j].start >= lists[j - 1].end;
    if (normalized) continue;
    any = true;
    for (int32_t g = 0; g < n_groups; ++g)
      n_g[(size_t)g] = std::max(n_g[(size_t)g], list_off[l * n_groups + g + 1] - list_off[l * n_groups + g]);
  }
  if (any && (rc = T.check_any_lists(ctx, n_g.data(), n_groups, "normalized lists, shorter lists or a smaller scale"))) return rc;
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, (int64_t)n_tracks * gat::kSignalWords, out_host);
}

// (not the fold: the words of a batch are copied out behind it, and an empty range writes nothing)
extern "C" int gat_sample_signal(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                 const gat_segment* pieces, const int32_t* values, const int64_t* piece_off,
                                 int32_t n_tracks, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_signal";
  if (!ctx || !P || !piece_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  SignalCall T = {who, pieces, values, piece_off, n_tracks};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  // lists that are not normalized (one unit a contig): as many segments on a contig as its region of the slab holds -- checked
  // again behind a batch for which the slab had to grow, before that batch is reduced
  int64_t checked_scale = 0;
  const auto check_slab = [&]() {
    if (sampled_lists_normalized(P) || checked_scale == P->cap_scale) return GAT_OK;
    std::vector<int64_t> n_g((size_t)P->n_contigs);
    for (int c = 0; c < P->n_contigs; ++c) n_g[(size_t)c] = P->h_units[(size_t)P->h_count_n_index[c]].slab_cap;
    checked_scale = P->cap_scale;
    return T.check_any_lists(ctx, n_g.data(), P->n_contigs, "n is what a contig's region of the sampler's slab holds; isochore keys "
                             "(normalized lists) or a smaller scale");
  };
  if ((rc = check_slab())) return rc;
  return call_frame(ctx, P, stats, [&](const Knobs& kn, gat_stats& local) {
    const int C = P->n_contigs;
    const int64_t S = sample_end - sample_begin;
    if (S == 0) return GAT_OK;                        // (no batch runs: nothing is written)
    const int urc = T.upload(ctx, kn, C, S);
    if (urc) return urc;
    return for_each_sampler_batch(ctx, P, kn, seed, sample_begin, S, local, BatchOpts(), [&](int64_t done, int64_t nb) {
      const size_t words = (size_t)(nb * n_tracks * gat::kSignalWords);
      if (words == 0) return GAT_OK;
      if (const int brc = check_slab()) return brc;
      if (T.out.d_out.n < words) HIPCHK(ctx, T.out.d_out.alloc(words));
      HIPCHK(ctx, hipMemsetAsync(T.out.d_out.p, 0, words * 8, ctx->stream));
      const int lrc = T.launch(ctx, kn, sampled_lists(P), nb, C, true);
      if (lrc) return lrc;
      HIPCHK(ctx, staged_d2h(ctx, out_host + done * n_tracks * gat::kSignalWords, T.out.d_out.p, words * 8));
      return GAT_OK;
    });
  });
}

// gat_list_bin_overlaps / gat_sample_bin_enrichment: k_local (gat_local.h) over caller-provided lists, or behind every batch.
// The tracks go up once per call (uint2, from anno_off[0]); the windows -- W bins of one (track, contig) and the slice of the
// track that reaches into them -- are made on the host per call, and only those a track reaches into: everywhere else v is
// 0.  The device buffers live for the call.
static const char* const kLocalWhy = "the overlap per bin is formed from disjoint pieces";
struct LocalCall {
  const char* who;
  const gat_segment* annos; const int64_t* anno_off; int32_t n_tracks; int64_t bin_size; const int64_t* bin_off;
  DevLists tracks;
  DevBuf<gat::LocalWindow> d_win;
  NullWordsOut out;
  std::vector<gat::LocalWindow> win;
  int64_t W = 0, L = 0;
  // what both entry points ask of the bins and the tracks
  int check(gat_ctx* ctx, int64_t n_groups) const {
    const int rc = check_bins(ctx, who, bin_size, bin_off, n_groups, "group");
    return rc ? rc : check_tracks(ctx, who, annos, anno_off, n_tracks, n_groups, kLocalWhy);
  }
  // the windows of a call (gat_local_windows.h) and the tracks, on the device
  int upload(gat_ctx* ctx, const Knobs& kn, int32_t n_groups, int64_t) {
    L = std::max<int64_t>(1, std::min<int64_t>(kn.local_lds_pieces, 8192));
    W = std::max<int64_t>(1, std::min<int64_t>(kn.local_window_bins, gat::local_max_window(ctx->max_lds, L)));
    if (!gat::local_build_windows(annos, anno_off, n_tracks, n_groups, bin_size, bin_off, W, win))
      return set_err(ctx, GAT_ERR_CAPACITY, "%s: more than 2^31 windows of %lld bins", who, (long long)W);
    const int rc = tracks.upload(ctx, annos, anno_off, (int64_t)n_tracks * n_groups);
    if (rc) return rc;
    HIPCHK(ctx, d_win.upload(win, ctx));
    return GAT_OK;
  }
  // one launch over n_lists x windows; store: the raw values per list, a row of every (track, bin) each, else the fold into
  // out's five words
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool store) const {
    if (win.empty() || n_lists == 0) return GAT_OK;
    gat::LocalArgs A;
    memset(&A, 0, sizeof(A));
    A.lists = lists;
    A.n_lists = (int32_t)n_lists;
    A.n_groups = n_groups;
    A.window_bins = (int32_t)W;
    A.lds_pieces = (int32_t)L;
    A.span32 = W * bin_size <= (int64_t)1 << 32 ? 1 : 0;
    A.bin_size = bin_size;
    A.list_stride = store ? (int64_t)n_tracks * bin_off[n_groups] : 0;
    A.win = d_win.p;
    A.annos = tracks.d_seg.p;
    A.obs = out.d_obs.p;
    A.out = out.d_out.p;
    const int64_t n_win = (int64_t)win.size();
    const int64_t lpb = kn.local_samples_per_block > 0 ? gat::run_per_block(n_lists, n_win, 0, kn.local_samples_per_block)
                                                       : gat::run_per_block(n_lists, n_win, 1024, gat::kNoRunCap);
    A.lists_per_block = (int32_t)lpb;
    const size_t lds = gat::local_lds_bytes(W, L, store);
    const dim3 grid((unsigned)n_win, (unsigned)((n_lists + lpb - 1) / lpb));
    return launch_store_or_fold(ctx, store, gat::k_local<true>, gat::k_local<false>, grid, gat::kLocalThreads, lds, A);
  }
};

extern "C" int gat_list_bin_overlaps(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                     const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int32_t n_groups,
                                     int64_t bin_size, const int64_t* bin_off, int64_t* out_host) {
  const char* who = "gat_list_bin_overlaps";
  if (!ctx || !list_off || !anno_off || !bin_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  LocalCall T = {who, annos, anno_off, n_tracks, bin_size, bin_off};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = check_caller_lists(ctx, who, "intervals", lists, list_off, n_lists, n_groups, kLocalWhy))) return rc;
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, (int64_t)n_tracks * bin_off[n_groups], out_host);
}

extern "C" int gat_sample_bin_enrichment(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                         const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                                         int64_t bin_size, const int64_t* bin_off, const int64_t* obs_host,
                                         int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_bin_enrichment";
  if (!ctx || !P || !anno_off || !bin_off || !obs_host || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  LocalCall T = {who, annos, anno_off, n_tracks, bin_size, bin_off};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  const int64_t S = sample_end - sample_begin, cells = (int64_t)n_tracks * bin_off[P->n_contigs];
  if ((rc = check_null_words(ctx, who, "bin_size", bin_size, "a smaller bin_size or fewer samples per call", S, obs_host, cells))) return rc;
  if ((rc = check_sampled_lists_normalized(ctx, who, P, "the overlap per bin needs normalized lists"))) return rc;
  return fold_over_sampled_batches(ctx, P, stats, seed, sample_begin, S, T, obs_host, cells, out_host);
}

// gat_list_pair_hits / gat_sample_pair_enrichment: k_pairs (gat_pairs.h) over caller-provided lists, or behind every batch.
// The tracks go up once per call (CSR, uint2); the device buffers live for the call.
static const char* const kPairsWhy = "the first interval that reaches a segment is searched for in it";
struct PairsCall {
  const char* who;
  const gat_segment* annos; const int64_t* anno_off; int32_t n_tracks;
  DevLists tracks;
  NullWordsOut out;
  // what both entry points ask of the tracks
  int check(gat_ctx* ctx, int64_t n_groups) const {
    if (n_tracks < 0 || n_tracks > gat::kPairsMaxTracks)
      return set_err(ctx, GAT_ERR_ARG, "%s: n_tracks %lld outside [0, %d]", who, (long long)n_tracks, gat::kPairsMaxTracks);
    if (n_tracks * std::max<int64_t>(1, n_groups) > (int64_t)INT32_MAX) return set_err(ctx, GAT_ERR_ARG, "%s: n_tracks %lld x %lld groups", who, (long long)n_tracks, (long long)n_groups);
    return check_track_lists(ctx, who, annos, anno_off, n_tracks, n_groups, kPairsWhy);
  }
  int upload(gat_ctx* ctx, const Knobs&, int32_t n_groups, int64_t) { return tracks.upload(ctx, annos, anno_off, (int64_t)n_tracks * n_groups); }
  // one launch over tiles x runs of n_lists lists; store: the raw counts per list, else the fold into out's five words.
  // The run: the knob's where it is set, else as long as leaves 4 096 workgroups -- three rounds of the five a compute unit holds: the
  // tiles of a call are not equally long, and a last round that is half empty costs as much as a full one -- but at least 8 lists
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool store) const {
    if (n_lists == 0 || n_tracks == 0 || n_groups == 0) return GAT_OK;
    gat::PairsArgs A;
    memset(&A, 0, sizeof(A));
    A.lists = lists;
    A.n_lists = (int32_t)n_lists;
    A.n_groups = n_groups;
    A.n_tracks = n_tracks;
    const int64_t L = gat::pairs_lds_pieces(std::max<int64_t>(0, kn.pairs_lds_pieces), n_groups);
    A.lds_pieces = (int32_t)L;
    A.annos = tracks.d_seg.p;
    A.anno_csr = tracks.d_csr.p;
    A.obs = out.d_obs.p;
    A.out = out.d_out.p;
    const int64_t n_tiles = gat::pairs_tiles(n_tracks);
    const int64_t lpb = kn.pairs_samples_per_block > 0 ? gat::run_per_block(n_lists, n_tiles, 0, kn.pairs_samples_per_block)
                                                       : gat::run_per_block(n_lists, n_tiles, 4096, gat::kNoRunCap);
    A.lists_per_block = (int32_t)lpb;
    const size_t lds = (size_t)gat::pairs_lds_bytes(L, n_groups);
    const dim3 grid((unsigned)n_tiles, (unsigned)((n_lists + lpb - 1) / lpb));
    return launch_store_or_fold(ctx, store, gat::k_pairs<true>, gat::k_pairs<false>, grid, gat::kPairsThreads, lds, A);
  }
};

extern "C" int gat_list_pair_hits(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                  const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks, int32_t n_groups,
                                  int64_t* out_host) {
  const char* who = "gat_list_pair_hits";
  if (!ctx || !list_off || !anno_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  PairsCall T = {who, annos, anno_off, n_tracks};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = check_caller_lists(ctx, who, "segments", lists, list_off, n_lists, n_groups, nullptr))) return rc;
  for (int64_t l = 0; l < n_lists; ++l)          // (a list's count of a pair is a 32-bit word on the device)
    if (list_off[(l + 1) * n_groups] - list_off[l * n_groups] > (int64_t)INT32_MAX)
      return set_err(ctx, GAT_ERR_CAPACITY, "%s: list %lld holds more than 2^31 - 1 segments", who, (long long)l);
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, gat::pairs_count(n_tracks), out_host);
}

extern "C" int gat_sample_pair_enrichment(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                          const gat_segment* annos, const int64_t* anno_off, int32_t n_tracks,
                                          const int64_t* obs_host, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_pair_enrichment";
  if (!ctx || !P || !anno_off) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  PairsCall T = {who, annos, anno_off, n_tracks};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  const int64_t S = sample_end - sample_begin, pairs = gat::pairs_count(n_tracks);
  if (pairs > 0 && (!obs_host || !out_host)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  const int64_t n_max = P->slab_stride;           // the most segments one sample can hold
  if (n_max > (int64_t)INT32_MAX) return set_err(ctx, GAT_ERR_CAPACITY, "%s: a sample can hold %lld segments, more than 2^31 - 1", who, (long long)n_max);
  if ((rc = check_null_words(ctx, who, "n_max", n_max, "fewer samples per call", S, obs_host, pairs))) return rc;
  return fold_over_sampled_batches(ctx, P, stats, seed, sample_begin, S, T, obs_host, pairs, out_host);
}

// gat_list_geneset_hits / gat_sample_geneset_enrichment: k_geneset_hits and k_geneset_terms (gat_geneset.h) over caller-provided
// lists, or behind every batch.  The pieces, their members and the terms go up once per call; the device buffers live for the call.
static const char* const kGenesetWhy = "the pieces a segment reaches are searched for in it";
// ids[b .. e) within [0, n_genes) and strictly ascending
static bool geneset_ids_ok(const int32_t* ids, int64_t b, int64_t e, int32_t n_genes) {
  for (int64_t m = b; m < e; ++m)
    if (ids[m] < 0 || ids[m] >= n_genes || (m > b && ids[m] <= ids[m - 1])) return false;
  return true;
}
// n + 1 offsets from 0, and the ids they index
static int geneset_upload_csr(gat_ctx* ctx, const int64_t* off, int64_t n, const int32_t* ids, DevBuf<int64_t>& d_off, DevBuf<int32_t>& d_ids) {
  const int64_t base = off[0], total = off[n] - base;
  HIPCHK(ctx, d_off.upload_built((size_t)n + 1, ctx, [&](int64_t* h) { for (int64_t k = 0; k <= n; ++k) h[k] = off[k] - base; }));
  HIPCHK(ctx, d_ids.upload_built((size_t)total, ctx, [&](int32_t* h) { memcpy(h, ids + base, (size_t)total * 4); }));
  return GAT_OK;
}
struct GenesetCall {
  const char* who;
  const gat_segment* pieces; const int64_t* piece_off; const int64_t* member_off; const int32_t* members; int32_t n_genes;
  const int64_t* term_off; const int32_t* term_genes; int32_t n_terms;
  DevLists d_pieces;
  DevBuf<int64_t> d_member_off, d_term_off;
  DevBuf<int32_t> d_members, d_term_genes;
  DevBuf<uint32_t> d_bitmaps;
  NullWordsOut out;
  int64_t chunk = 0;         // lists whose bitmaps d_bitmaps holds
  // what both entry points ask of the genes and the terms
  int check(gat_ctx* ctx, int64_t n_groups) const {
    if (n_genes < 0 || n_genes > gat::kGenesetMaxGenes)
      return set_err(ctx, GAT_ERR_ARG, "%s: n_genes %d outside [0, %d]", who, n_genes, gat::kGenesetMaxGenes);
    if (n_terms < 0) return set_err(ctx, GAT_ERR_ARG, "%s: n_terms %d is negative", who, n_terms);
    int rc;
    if ((rc = check_list_offsets(ctx, who, "piece_off", "pieces", piece_off, n_groups))) return rc;
    const int64_t n_pieces = piece_off[n_groups] - piece_off[0];
    if (n_pieces > 0 && !pieces) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    if ((rc = check_normalized(ctx, who, "gene pieces", pieces, piece_off, 1, (int32_t)n_groups, kGenesetWhy))) return rc;
    if (member_off[0] < 0) return set_err(ctx, GAT_ERR_ARG, "%s: member_off[0] < 0", who);
    for (int64_t j = 0; j < n_pieces; ++j) {
      if (member_off[j + 1] < member_off[j]) return set_err(ctx, GAT_ERR_ARG, "%s: member_off decreases at piece %lld", who, (long long)j);
      if (member_off[j + 1] == member_off[j]) return set_err(ctx, GAT_ERR_ARG, "%s: piece %lld has no member", who, (long long)j);
    }
    if (member_off[n_pieces] > member_off[0] && !members) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    for (int64_t j = 0; j < n_pieces; ++j)
      if (!geneset_ids_ok(members, member_off[j], member_off[j + 1], n_genes))
        return set_err(ctx, GAT_ERR_ARG, "%s: the members of piece %lld are not strictly ascending gene ids in [0, %d)", who, (long long)j, n_genes);
    if (term_off[0] < 0) return set_err(ctx, GAT_ERR_ARG, "%s: term_off[0] < 0", who);
    for (int64_t t = 0; t < n_terms; ++t)
      if (term_off[t + 1] < term_off[t]) return set_err(ctx, GAT_ERR_ARG, "%s: term_off decreases at term %lld", who, (long long)t);
    if (term_off[n_terms] > term_off[0] && !term_genes) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    for (int64_t t = 0; t < n_terms; ++t)
      if (!geneset_ids_ok(term_genes, term_off[t], term_off[t + 1], n_genes))
        return set_err(ctx, GAT_ERR_ARG, "%s: the genes of term %lld are not strictly ascending gene ids in [0, %d)", who, (long long)t, n_genes);
    return GAT_OK;
  }
  // the genes and the terms on the device, and the bitmaps of as many lists as a quarter of GAT_SLAB_BYTES holds -- at most
  // 256 MB, at least one list's, no more than the call's n_lists
  int upload(gat_ctx* ctx, const Knobs& kn, int32_t n_groups, int64_t n_lists) {
    int rc;
    if ((rc = d_pieces.upload(ctx, pieces, piece_off, n_groups))) return rc;
    const int64_t n_pieces = piece_off[n_groups] - piece_off[0];
    if ((rc = geneset_upload_csr(ctx, member_off, n_pieces, members, d_member_off, d_members))) return rc;
    if ((rc = geneset_upload_csr(ctx, term_off, n_terms, term_genes, d_term_off, d_term_genes))) return rc;
    const int64_t row = gat::geneset_bitmap_words(n_genes) * 4;
    const double budget = std::min(kn.slab_bytes / 4.0, 256.0 * 1024 * 1024);
    chunk = std::max<int64_t>(1, std::min<int64_t>(n_lists, (int64_t)(budget / (double)row)));
    HIPCHK(ctx, d_bitmaps.alloc((size_t)(chunk * row / 4)));
    return GAT_OK;
  }
  // n_lists lists in chunks of `chunk`: k_geneset_hits writes a chunk's bitmaps, k_geneset_terms reads them.  store: the raw counts
  // per list (row `first + i` of out.d_out), else the fold into out's five words.  The runs: the knob's where it is set, else
  // as long as leaves 2 048 workgroups (eight for each of 256 compute units) but at least 16 lists
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool store) const {
    if (n_lists == 0 || n_terms == 0) return GAT_OK;
    const int64_t W = gat::geneset_bitmap_words(n_genes);
    const int64_t L = gat::geneset_lds_pieces(kn.geneset_lds_pieces, n_groups);
    const int64_t tile = std::min<int64_t>(gat::kGenesetMaxTermTile, std::max<int64_t>(1, kn.geneset_term_tile));
    const int64_t n_tiles = (n_terms + tile - 1) / tile;
    const int64_t knob_run = kn.geneset_samples_per_block;
    for (int64_t first = 0; first < n_lists; first += chunk) {
      const int64_t n = std::min(chunk, n_lists - first);
      gat::GenesetHitsArgs H;
      memset(&H, 0, sizeof(H));
      H.lists = lists;
      H.list_begin = (int32_t)first;
      H.n_lists = (int32_t)n;
      H.n_groups = n_groups;
      H.lds_pieces = (int32_t)L;
      H.bm_words = (int32_t)W;
      H.pieces = d_pieces.d_seg.p;
      H.piece_csr = d_pieces.d_csr.p;
      H.member_off = d_member_off.p;
      H.members = d_members.p;
      H.bitmaps = d_bitmaps.p;
      const int64_t run_h = knob_run > 0 ? gat::run_per_block(n, 1, 0, knob_run) : gat::run_per_block(n, 1, 2048, gat::kNoRunCap);
      H.lists_per_block = (int32_t)run_h;
      const size_t lds_h = (size_t)(W + (int64_t)n_groups * L) * 4;
      HIPCHK(ctx, hipFuncSetAttribute((const void*)gat::k_geneset_hits, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_h));
      hipLaunchKernelGGL(gat::k_geneset_hits, dim3((unsigned)((n + run_h - 1) / run_h)), dim3(gat::kGenesetThreads), lds_h, ctx->stream, H);
      HIPCHK(ctx, hipGetLastError());

      gat::GenesetTermsArgs T;
      memset(&T, 0, sizeof(T));
      T.bitmaps = d_bitmaps.p;
      T.list_begin = (int32_t)first;
      T.n_lists = (int32_t)n;
      T.bm_words = (int32_t)W;
      T.term_tile = (int32_t)tile;
      T.n_terms = n_terms;
      T.term_off = d_term_off.p;
      T.term_genes = d_term_genes.p;
      T.obs = out.d_obs.p;
      T.out = out.d_out.p;
      const int64_t run_t = knob_run > 0 ? gat::run_per_block(n, n_tiles, 0, knob_run) : gat::run_per_block(n, n_tiles, 2048, gat::kNoRunCap);
      T.lists_per_block = (int32_t)run_t;
      const dim3 grid((unsigned)n_tiles, (unsigned)((n + run_t - 1) / run_t));
      if (store) hipLaunchKernelGGL(gat::k_geneset_terms<true>, grid, dim3(gat::kGenesetThreads), (size_t)W * 4, ctx->stream, T);
      else hipLaunchKernelGGL(gat::k_geneset_terms<false>, grid, dim3(gat::kGenesetThreads), (size_t)W * 4, ctx->stream, T);
      HIPCHK(ctx, hipGetLastError());
    }
    return GAT_OK;
  }
};

extern "C" int gat_list_geneset_hits(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                     const gat_segment* pieces, const int64_t* piece_off, const int64_t* member_off, const int32_t* members,
                                     int32_t n_genes, const int64_t* term_off, const int32_t* term_genes, int32_t n_terms,
                                     int32_t n_groups, int64_t* out_host) {
  const char* who = "gat_list_geneset_hits";
  if (!ctx || !list_off || !piece_off || !member_off || !term_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  GenesetCall T = {who, pieces, piece_off, member_off, members, n_genes, term_off, term_genes, n_terms};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = check_caller_lists(ctx, who, "segments", lists, list_off, n_lists, n_groups, nullptr))) return rc;
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, n_terms, out_host);
}

extern "C" int gat_sample_geneset_enrichment(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                             const gat_segment* pieces, const int64_t* piece_off, const int64_t* member_off,
                                             const int32_t* members, int32_t n_genes, const int64_t* term_off, const int32_t* term_genes,
                                             int32_t n_terms, const int64_t* obs_host, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_geneset_enrichment";
  if (!ctx || !P || !piece_off || !member_off || !term_off) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  GenesetCall T = {who, pieces, piece_off, member_off, members, n_genes, term_off, term_genes, n_terms};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  const int64_t S = sample_end - sample_begin;
  if (n_terms > 0 && (!obs_host || !out_host)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if ((rc = check_null_words(ctx, who, "n_genes", n_genes, "fewer samples per call", S, obs_host, n_terms))) return rc;
  return fold_over_sampled_batches(ctx, P, stats, seed, sample_begin, S, T, obs_host, n_terms, out_host);
}

// gat_list_profile / gat_sample_profile_enrichment: k_profile (gat_profile.h) over caller-provided lists, or behind every batch.
// The anchors go up once per call (positions, strands, offsets from anchor_off[0]); the device buffers live for the call.
static const char* const kProfileWhy = "a base counts once per anchor: the profile is formed from disjoint segments";
struct ProfileCall {
  const char* who;
  const uint32_t* pos; const uint8_t* minus; const int64_t* off;
  int32_t n_tracks; int64_t bin_size; int32_t half_bins; int mode;
  DevBuf<uint32_t> d_pos;
  DevBuf<uint8_t> d_minus;
  DevBuf<int64_t> d_off;
  NullWordsOut out;
  int64_t longest = 0;        // the most anchors of a (track, group)
  int64_t most_bases = 0;     // the largest K_t * bin_size of a track, what a value can reach (check)
  // what both entry points ask of the bins and the anchors (tracks of points, not of intervals: the checks are its own)
  int check(gat_ctx* ctx, int64_t n_groups) {
    if (bin_size < 1 || bin_size > (int64_t)1 << 31) return set_err(ctx, GAT_ERR_ARG, "%s: bin_size %lld outside [1, 2^31]", who, (long long)bin_size);
    if (half_bins < 1 || 2 * (int64_t)half_bins > GAT_PROFILE_MAX_BINS)
      return set_err(ctx, GAT_ERR_ARG, "%s: half_bins %d outside [1, %d]", who, half_bins, GAT_PROFILE_MAX_BINS / 2);
    if (half_bins * bin_size > (int64_t)1 << 31)
      return set_err(ctx, GAT_ERR_ARG, "%s: half_bins * bin_size = %d * %lld is more than 2^31", who, half_bins, (long long)bin_size);
    if (mode != GAT_PROFILE_BASES && mode != GAT_PROFILE_MIDPOINTS)
      return set_err(ctx, GAT_ERR_ARG, "%s: mode %d is neither GAT_PROFILE_BASES nor GAT_PROFILE_MIDPOINTS", who, mode);
    if (n_tracks < 0 || (int64_t)n_tracks * std::max<int64_t>(1, n_groups) > (int64_t)INT32_MAX)
      return set_err(ctx, GAT_ERR_ARG, "%s: n_tracks %d", who, n_tracks);
    const int64_t n = (int64_t)n_tracks * n_groups;
    int rc;
    if ((rc = check_list_offsets(ctx, who, "anchor_off", "anchors", off, n))) return rc;
    if (off[n] > off[0] && (!pos || !minus)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    most_bases = 0;
    for (int64_t t = 0; t < n_tracks; ++t) {
      for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t b = off[t * n_groups + g], e = off[t * n_groups + g + 1];
        for (int64_t k = b; k < e; ++k) {
          if (minus[k] > 1)
            return set_err(ctx, GAT_ERR_ARG, "%s: anchor track %lld, group %lld: anchor_minus %d at anchor %lld is neither 0 nor 1", who,
                           (long long)t, (long long)g, (int)minus[k], (long long)(k - b));
          if (k == b) continue;
          const int64_t before = (int64_t)pos[k - 1] * 2 + minus[k - 1], here = (int64_t)pos[k] * 2 + minus[k];
          if (here == before)
            return set_err(ctx, GAT_ERR_ARG, "%s: anchor track %lld, group %lld repeats an anchor (position, strand) at anchor %lld", who,
                           (long long)t, (long long)g, (long long)(k - b));
          if (here < before)
            return set_err(ctx, GAT_ERR_ARG, "%s: anchor track %lld, group %lld is out of order at anchor %lld (ascending by position, "
                           "plus before minus at one position)", who, (long long)t, (long long)g, (long long)(k - b));
        }
      }
      most_bases = std::max<int64_t>(most_bases, (off[(t + 1) * n_groups] - off[t * n_groups]) * bin_size);
    }
    return GAT_OK;
  }
  // K_t * bin_size of every track below 2^32 -- a value is a 32-bit word on the device -- and its square times S below 2^64
  int check_words(gat_ctx* ctx, int64_t S, const int64_t* obs_host, int64_t cells) const {
    if (most_bases >= (int64_t)1 << 32)
      return set_err(ctx, GAT_ERR_ARG, "%s: anchors * bin_size = %lld of a track does not fit 32 bits: fewer anchors per track or a smaller bin_size",
                     who, (long long)most_bases);
    return check_null_words(ctx, who, "anchors * bin_size", most_bases, "fewer anchors per track, a smaller bin_size or fewer samples per call",
                            S, obs_host, cells);
  }
  int upload(gat_ctx* ctx, const Knobs&, int32_t n_groups, int64_t) {
    const int64_t n = (int64_t)n_tracks * n_groups, base = off[0], total = off[n] - base;
    std::vector<int64_t> h_off((size_t)n + 1);
    longest = 0;
    for (int64_t l = 0; l <= n; ++l) {
      h_off[(size_t)l] = off[l] - base;
      if (l) longest = std::max(longest, off[l] - off[l - 1]);
    }
    HIPCHK(ctx, d_pos.alloc((size_t)total));
    HIPCHK(ctx, d_minus.alloc((size_t)total));
    if (total > 0) {
      HIPCHK(ctx, staged_h2d(ctx, d_pos.p, pos + base, (size_t)total * 4));
      HIPCHK(ctx, staged_h2d(ctx, d_minus.p, minus + base, (size_t)total));
    }
    HIPCHK(ctx, d_off.upload(h_off, ctx));
    HIPCHK(ctx, stage_flush(ctx));                    // (h_off goes away with this frame)
    return GAT_OK;
  }
  // one launch over tracks x runs of n_lists lists; store: the raw values per list, else the fold into out's five words
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool store) const {
    if (n_lists == 0 || n_tracks == 0 || n_groups == 0 || longest == 0) return GAT_OK;
    gat::ProfileArgs A;
    memset(&A, 0, sizeof(A));
    const int64_t bins = 2 * (int64_t)half_bins;
    const int64_t L = gat::profile_lds_anchors(std::max<int64_t>(0, kn.profile_lds_anchors), longest, ctx->max_lds, bins, n_groups);
    A.lists = lists;
    A.n_lists = (int32_t)n_lists;
    A.n_groups = n_groups;
    A.n_tracks = n_tracks;
    A.bins = (int32_t)bins;
    A.lds_anchors = (int32_t)L;
    A.midpoints = mode == GAT_PROFILE_MIDPOINTS ? 1 : 0;
    A.bin_size = bin_size;
    A.reach = half_bins * bin_size;
    A.pos = d_pos.p;
    A.minus = d_minus.p;
    A.anchor_off = d_off.p;
    A.obs = out.d_obs.p;
    A.out = out.d_out.p;
    // the run: the knob's where it is set, else as long as leaves 8 192 workgroups -- four rounds of the eight a compute unit holds at
    // 100 bins: the lists of a run are not equally long, and runs of 4 and 16 were measured faster than runs of 49 and 64 there
    // (profiles/r22_profile.txt) -- but at least 8 lists: a workgroup's fixed cost is the flush of its bins; and a list for every
    // wave in every round: a run of 10 is three rounds for two of the four waves and two for the others, measured 1.17 x a run of 16
    const int64_t lpb = kn.profile_samples_per_block > 0
                            ? gat::run_per_block(n_lists, n_tracks, 0, kn.profile_samples_per_block)
                            : (gat::run_per_block(n_lists, n_tracks, 8192, gat::kNoRunCap) + gat::kProfileWaves - 1) / gat::kProfileWaves * gat::kProfileWaves;
    A.lists_per_block = (int32_t)lpb;
    const size_t lds = (size_t)gat::profile_lds_bytes(bins, L, n_groups, store);
    const dim3 grid((unsigned)n_tracks, (unsigned)((n_lists + lpb - 1) / lpb));
    return launch_store_or_fold(ctx, store, gat::k_profile<true>, gat::k_profile<false>, grid, gat::kProfileThreads, lds, A);
  }
};

extern "C" int gat_list_profile(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                const uint32_t* anchor_pos, const uint8_t* anchor_minus, const int64_t* anchor_off,
                                int32_t n_tracks, int32_t n_groups, int64_t bin_size, int32_t half_bins, int mode, int64_t* out_host) {
  const char* who = "gat_list_profile";
  if (!ctx || !list_off || !anchor_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  ProfileCall T = {who, anchor_pos, anchor_minus, anchor_off, n_tracks, bin_size, half_bins, mode};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = T.check_words(ctx, 1, nullptr, 0))) return rc;
  if ((rc = check_caller_lists(ctx, who, "intervals", lists, list_off, n_lists, n_groups, kProfileWhy))) return rc;
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, (int64_t)n_tracks * 2 * half_bins, out_host);
}

extern "C" int gat_sample_profile_enrichment(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                             const uint32_t* anchor_pos, const uint8_t* anchor_minus, const int64_t* anchor_off,
                                             int32_t n_tracks, int64_t bin_size, int32_t half_bins, int mode,
                                             const int64_t* obs_host, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_profile_enrichment";
  if (!ctx || !P || !anchor_off) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  ProfileCall T = {who, anchor_pos, anchor_minus, anchor_off, n_tracks, bin_size, half_bins, mode};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  const int64_t S = sample_end - sample_begin, cells = (int64_t)n_tracks * 2 * half_bins;
  if (cells > 0 && (!obs_host || !out_host)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if ((rc = T.check_words(ctx, S, obs_host, cells))) return rc;
  if ((rc = check_sampled_lists_normalized(ctx, who, P, "the profile needs normalized lists"))) return rc;
  return fold_over_sampled_batches(ctx, P, stats, seed, sample_begin, S, T, obs_host, cells, out_host);
}

// gat_list_reldist / gat_sample_reldist_enrichment: k_reldist (gat_reldist.h) over caller-provided lists, or behind every batch.
// The points go up once per call (positions, offsets from point_off[0]); the device buffers live for the call.
struct ReldistCall {
  const char* who;
  const uint32_t* pos; const int64_t* off;
  int32_t n_tracks; int32_t n_bins;
  DevBuf<uint32_t> d_pos;
  DevBuf<int64_t> d_off;
  NullWordsOut out;
  int64_t longest = 0;        // the most points of a (track, group)
  int64_t values() const { return (int64_t)n_bins + GAT_RELDIST_EXTRA; }
  // what both entry points ask of the bins and the points (tracks of points, not of intervals: the checks are its own)
  int check(gat_ctx* ctx, int64_t n_groups) const {
    if (n_bins < 1 || n_bins > GAT_RELDIST_MAX_BINS) return set_err(ctx, GAT_ERR_ARG, "%s: n_bins %d outside [1, %d]", who, n_bins, GAT_RELDIST_MAX_BINS);
    if (n_tracks < 0 || (int64_t)n_tracks * std::max<int64_t>(1, n_groups) > (int64_t)INT32_MAX)
      return set_err(ctx, GAT_ERR_ARG, "%s: n_tracks %d", who, n_tracks);
    const int64_t n = (int64_t)n_tracks * n_groups;
    int rc;
    if ((rc = check_list_offsets(ctx, who, "point_off", "points", off, n))) return rc;
    if (off[n] > off[0] && !pos) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    for (int64_t t = 0; t < n_tracks; ++t)
      for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t b = off[t * n_groups + g], e = off[t * n_groups + g + 1];
        for (int64_t k = b + 1; k < e; ++k)
          if (pos[k] <= pos[k - 1])
            return set_err(ctx, GAT_ERR_ARG, "%s: point track %lld, group %lld is not strictly ascending at point %lld", who,
                           (long long)t, (long long)g, (long long)(k - b));
      }
    return GAT_OK;
  }
  int upload(gat_ctx* ctx, const Knobs&, int32_t n_groups, int64_t) {
    const int64_t n = (int64_t)n_tracks * n_groups, base = off[0], total = off[n] - base;
    std::vector<int64_t> h_off((size_t)n + 1);
    longest = 0;
    for (int64_t l = 0; l <= n; ++l) {
      h_off[(size_t)l] = off[l] - base;
      if (l) longest = std::max(longest, off[l] - off[l - 1]);
    }
    HIPCHK(ctx, d_pos.alloc((size_t)total));
    if (total > 0) HIPCHK(ctx, staged_h2d(ctx, d_pos.p, pos + base, (size_t)total * 4));
    HIPCHK(ctx, d_off.upload(h_off, ctx));
    HIPCHK(ctx, stage_flush(ctx));                    // (h_off goes away with this frame)
    return GAT_OK;
  }
  // one launch over tracks x runs of n_lists lists; store: the raw values per list, else the fold into out's five words.  (A
  // call without a point still counts its segments: outside.)
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool store) const {
    if (n_lists == 0 || n_tracks == 0 || n_groups == 0) return GAT_OK;
    gat::ReldistArgs A;
    memset(&A, 0, sizeof(A));
    const int64_t L = gat::reldist_lds_points(std::max<int64_t>(0, kn.reldist_lds_points), longest, ctx->max_lds, n_bins, n_groups);
    A.lists = lists;
    A.n_lists = (int32_t)n_lists;
    A.n_groups = n_groups;
    A.n_tracks = n_tracks;
    A.bins = n_bins;
    A.lds_points = (int32_t)L;
    A.pos = d_pos.p;
    A.point_off = d_off.p;
    A.obs = out.d_obs.p;
    A.out = out.d_out.p;
    // the run: the knob's where it is set, else k_profile's rule, whose layout and fixed cost per workgroup (the flush of its
    // cells) this kernel shares: as long as leaves 8 192 workgroups, at least 8 lists, and a list for every wave in every round
    const int64_t lpb = kn.reldist_samples_per_block > 0
                            ? gat::run_per_block(n_lists, n_tracks, 0, kn.reldist_samples_per_block)
                            : (gat::run_per_block(n_lists, n_tracks, 8192, gat::kNoRunCap) + gat::kReldistWaves - 1) / gat::kReldistWaves * gat::kReldistWaves;
    A.lists_per_block = (int32_t)lpb;
    const size_t lds = (size_t)gat::reldist_lds_bytes(n_bins, L, n_groups, store);
    const dim3 grid((unsigned)n_tracks, (unsigned)((n_lists + lpb - 1) / lpb));
    return launch_store_or_fold(ctx, store, gat::k_reldist<true>, gat::k_reldist<false>, grid, gat::kReldistThreads, lds, A);
  }
};

extern "C" int gat_list_reldist(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                const uint32_t* point_pos, const int64_t* point_off, int32_t n_tracks, int32_t n_groups,
                                int32_t n_bins, int64_t* out_host) {
  const char* who = "gat_list_reldist";
  if (!ctx || !list_off || !point_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  ReldistCall T = {who, point_pos, point_off, n_tracks, n_bins};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = check_caller_lists(ctx, who, "segments", lists, list_off, n_lists, n_groups, nullptr))) return rc;
  // a value is a 32-bit word on the device, and the area's route takes n < 2^31: the segments of a list over all its groups
  for (int64_t l = 0; l < n_lists; ++l)
    if (list_off[(l + 1) * n_groups] - list_off[l * n_groups] > (int64_t)INT32_MAX)
      return set_err(ctx, GAT_ERR_ARG, "%s: list %lld has more than 2^31 - 1 segments over its groups", who, (long long)l);
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, (int64_t)n_tracks * T.values(), out_host);
}

extern "C" int gat_sample_reldist_enrichment(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                             const uint32_t* point_pos, const int64_t* point_off, int32_t n_tracks, int32_t n_bins,
                                             const int64_t* obs_host, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_reldist_enrichment";
  if (!ctx || !P || !point_off) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  ReldistCall T = {who, point_pos, point_off, n_tracks, n_bins};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  const int64_t S = sample_end - sample_begin, cells = (int64_t)n_tracks * T.values();
  if (cells > 0 && (!obs_host || !out_host)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  const int64_t n_max = P->slab_stride;           // the most segments one sample can hold
  if (n_max > (int64_t)INT32_MAX) return set_err(ctx, GAT_ERR_CAPACITY, "%s: a sample can hold %lld segments, more than 2^31 - 1", who, (long long)n_max);
  // a count is at most n_max, the area at most GAT_RELDIST_AREA_SCALE
  if ((rc = check_null_words(ctx, who, "max(10^6, n_max)", std::max<int64_t>(GAT_RELDIST_AREA_SCALE, n_max), "fewer samples per call", S, obs_host, cells))) return rc;
  return fold_over_sampled_batches(ctx, P, stats, seed, sample_begin, S, T, obs_host, cells, out_host);
}

// gat_list_metagene / gat_sample_metagene_enrichment: k_metagene (gat_metagene.h) over caller-provided lists, or behind every
// batch.  The features go up once per call (starts, ends, the prefix maximum of the ends built here, strands, offsets from
// feat_off[0]); the device buffers live for the call.
static const char* const kMetageneWhy = "a base counts once per feature: the metagene is formed from disjoint segments";
struct MetageneCall {
  const char* who;
  const uint32_t* fs; const uint32_t* fe; const uint8_t* minus; const int64_t* off;
  int32_t n_tracks; int32_t body_bins; int32_t flank_bins; int64_t flank_bin_size; int mode;
  DevBuf<uint32_t> d_fs, d_fe, d_pm;
  DevBuf<uint8_t> d_minus;
  DevBuf<int64_t> d_off;
  NullWordsOut out;
  int64_t longest = 0;        // the most features of a (track, group)
  int64_t most = 0;           // what a value can reach: the larger of K_t * w (with flanks) and sum_f ceil(len_f / Bb), over the tracks (check)
  int64_t bins() const { return 2 * (int64_t)flank_bins + body_bins; }
  // what both entry points ask of the bins and the features (tracks of stranded intervals that may overlap: the checks are its own)
  int check(gat_ctx* ctx, int64_t n_groups) {
    if (body_bins < 1) return set_err(ctx, GAT_ERR_ARG, "%s: body_bins %d is less than 1", who, body_bins);
    if (flank_bins < 0) return set_err(ctx, GAT_ERR_ARG, "%s: flank_bins %d is negative", who, flank_bins);
    if (bins() > GAT_METAGENE_MAX_BINS)
      return set_err(ctx, GAT_ERR_ARG, "%s: 2 * flank_bins + body_bins = %lld is more than %d", who, (long long)bins(), GAT_METAGENE_MAX_BINS);
    if (flank_bin_size < 1 || flank_bin_size > (int64_t)1 << 31)
      return set_err(ctx, GAT_ERR_ARG, "%s: flank_bin_size %lld outside [1, 2^31]", who, (long long)flank_bin_size);
    if (flank_bins * flank_bin_size > (int64_t)1 << 31)
      return set_err(ctx, GAT_ERR_ARG, "%s: flank_bins * flank_bin_size = %d * %lld is more than 2^31", who, flank_bins, (long long)flank_bin_size);
    if (mode != GAT_METAGENE_BASES && mode != GAT_METAGENE_MIDPOINTS)
      return set_err(ctx, GAT_ERR_ARG, "%s: mode %d is neither GAT_METAGENE_BASES nor GAT_METAGENE_MIDPOINTS", who, mode);
    if (n_tracks < 0 || (int64_t)n_tracks * std::max<int64_t>(1, n_groups) > (int64_t)INT32_MAX)
      return set_err(ctx, GAT_ERR_ARG, "%s: n_tracks %d", who, n_tracks);
    const int64_t n = (int64_t)n_tracks * n_groups;
    int rc;
    if ((rc = check_list_offsets(ctx, who, "feat_off", "features", off, n))) return rc;
    if (off[n] > off[0] && (!fs || !fe || !minus)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
    most = 0;
    for (int64_t t = 0; t < n_tracks; ++t) {
      int64_t body = 0;       // sum_f ceil(len_f / Bb) < 2^31 * 2^32: no overflow
      for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t b = off[t * n_groups + g], e = off[t * n_groups + g + 1];
        for (int64_t k = b; k < e; ++k) {
          if (fe[k] <= fs[k])
            return set_err(ctx, GAT_ERR_ARG, "%s: feature track %lld, group %lld: feature %lld is empty (end <= start)", who,
                           (long long)t, (long long)g, (long long)(k - b));
          if (minus[k] > 1)
            return set_err(ctx, GAT_ERR_ARG, "%s: feature track %lld, group %lld: feat_minus %d at feature %lld is neither 0 nor 1", who,
                           (long long)t, (long long)g, (int)minus[k], (long long)(k - b));
          body += ((int64_t)(fe[k] - fs[k]) + body_bins - 1) / body_bins;
          if (k == b) continue;
          const bool same = fs[k] == fs[k - 1] && fe[k] == fe[k - 1] && minus[k] == minus[k - 1];
          if (same)
            return set_err(ctx, GAT_ERR_ARG, "%s: feature track %lld, group %lld repeats a feature (start, end, strand) at feature %lld", who,
                           (long long)t, (long long)g, (long long)(k - b));
          const bool after = fs[k] != fs[k - 1] ? fs[k] > fs[k - 1] : fe[k] != fe[k - 1] ? fe[k] > fe[k - 1] : minus[k] > minus[k - 1];
          if (!after)
            return set_err(ctx, GAT_ERR_ARG, "%s: feature track %lld, group %lld is out of order at feature %lld (ascending by start, "
                           "then end, plus before minus)", who, (long long)t, (long long)g, (long long)(k - b));
        }
      }
      const int64_t flank = flank_bins > 0 ? (off[(t + 1) * n_groups] - off[t * n_groups]) * flank_bin_size : 0;
      most = std::max<int64_t>(most, std::max(flank, body));
    }
    return GAT_OK;
  }
  // the most of a cell below 2^32 -- a value is a 32-bit word on the device -- and its square times S below 2^64
  int check_words(gat_ctx* ctx, int64_t S, const int64_t* obs_host, int64_t cells) const {
    if (most >= (int64_t)1 << 32)
      return set_err(ctx, GAT_ERR_ARG, "%s: the bases one bin of a track can hold, %lld, do not fit 32 bits: fewer features per track, a "
                     "smaller flank_bin_size or more body_bins", who, (long long)most);
    return check_null_words(ctx, who, "bases per bin", most, "fewer features per track, a smaller flank_bin_size, more body_bins or fewer samples per call",
                            S, obs_host, cells);
  }
  int upload(gat_ctx* ctx, const Knobs&, int32_t n_groups, int64_t) {
    const int64_t n = (int64_t)n_tracks * n_groups, base = off[0], total = off[n] - base;
    std::vector<int64_t> h_off((size_t)n + 1);
    std::vector<uint32_t> h_pm((size_t)total);
    longest = 0;
    for (int64_t l = 0; l <= n; ++l) {
      h_off[(size_t)l] = off[l] - base;
      if (!l) continue;
      longest = std::max(longest, off[l] - off[l - 1]);
      uint32_t m = 0u;
      for (int64_t k = off[l - 1]; k < off[l]; ++k) h_pm[(size_t)(k - base)] = m = std::max(m, fe[k]);
    }
    HIPCHK(ctx, d_fs.alloc((size_t)total));
    HIPCHK(ctx, d_fe.alloc((size_t)total));
    HIPCHK(ctx, d_pm.alloc((size_t)total));
    HIPCHK(ctx, d_minus.alloc((size_t)total));
    if (total > 0) {
      HIPCHK(ctx, staged_h2d(ctx, d_fs.p, fs + base, (size_t)total * 4));
      HIPCHK(ctx, staged_h2d(ctx, d_fe.p, fe + base, (size_t)total * 4));
      HIPCHK(ctx, staged_h2d(ctx, d_pm.p, h_pm.data(), (size_t)total * 4));
      HIPCHK(ctx, staged_h2d(ctx, d_minus.p, minus + base, (size_t)total));
    }
    HIPCHK(ctx, d_off.upload(h_off, ctx));
    HIPCHK(ctx, stage_flush(ctx));                    // (h_off and h_pm go away with this frame)
    return GAT_OK;
  }
  // one launch over tracks x runs of n_lists lists; store: the raw values per list, else the fold into out's five words
  int launch(gat_ctx* ctx, const Knobs& kn, const gat::ListSet& lists, int64_t n_lists, int32_t n_groups, bool store) const {
    if (n_lists == 0 || n_tracks == 0 || n_groups == 0 || longest == 0) return GAT_OK;
    gat::MetageneArgs A;
    memset(&A, 0, sizeof(A));
    const int64_t L = gat::metagene_lds_features(std::max<int64_t>(0, kn.metagene_lds_features), longest, ctx->max_lds, bins(), n_groups);
    A.lists = lists;
    A.n_lists = (int32_t)n_lists;
    A.n_groups = n_groups;
    A.n_tracks = n_tracks;
    A.bins = (int32_t)bins();
    A.body_bins = body_bins;
    A.flank_bins = flank_bins;
    A.lds_features = (int32_t)L;
    A.midpoints = mode == GAT_METAGENE_MIDPOINTS ? 1 : 0;
    A.flank_bin_size = flank_bin_size;
    A.flank = flank_bins * flank_bin_size;
    A.fs = d_fs.p;
    A.fe = d_fe.p;
    A.pm = d_pm.p;
    A.minus = d_minus.p;
    A.feat_off = d_off.p;
    A.obs = out.d_obs.p;
    A.out = out.d_out.p;
    // the run: the knob's where it is set, else k_profile's rule, whose layout and fixed cost per workgroup (the flush of its
    // bins) this kernel shares: as long as leaves 8 192 workgroups, at least 8 lists, and a list for every wave in every round
    const int64_t lpb = kn.metagene_samples_per_block > 0
                            ? gat::run_per_block(n_lists, n_tracks, 0, kn.metagene_samples_per_block)
                            : (gat::run_per_block(n_lists, n_tracks, 8192, gat::kNoRunCap) + gat::kMetageneWaves - 1) / gat::kMetageneWaves * gat::kMetageneWaves;
    A.lists_per_block = (int32_t)lpb;
    const size_t lds = (size_t)gat::metagene_lds_bytes(bins(), L, n_groups, store);
    const dim3 grid((unsigned)n_tracks, (unsigned)((n_lists + lpb - 1) / lpb));
    return launch_store_or_fold(ctx, store, gat::k_metagene<true>, gat::k_metagene<false>, grid, gat::kMetageneThreads, lds, A);
  }
};

extern "C" int gat_list_metagene(gat_ctx* ctx, const gat_segment* lists, const int64_t* list_off, int64_t n_lists,
                                 const uint32_t* feat_start, const uint32_t* feat_end, const uint8_t* feat_minus, const int64_t* feat_off,
                                 int32_t n_tracks, int32_t n_groups, int32_t body_bins, int32_t flank_bins, int64_t flank_bin_size,
                                 int mode, int64_t* out_host) {
  const char* who = "gat_list_metagene";
  if (!ctx || !list_off || !feat_off || !out_host) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  MetageneCall T = {who, feat_start, feat_end, feat_minus, feat_off, n_tracks, body_bins, flank_bins, flank_bin_size, mode};
  int rc;
  if ((rc = check_list_counts(ctx, who, n_lists, n_groups))) return rc;
  if ((rc = T.check(ctx, n_groups))) return rc;
  if ((rc = T.check_words(ctx, 1, nullptr, 0))) return rc;
  if ((rc = check_caller_lists(ctx, who, "intervals", lists, list_off, n_lists, n_groups, kMetageneWhy))) return rc;
  return store_over_caller_lists(ctx, T, lists, list_off, n_lists, n_groups, (int64_t)n_tracks * T.bins(), out_host);
}

extern "C" int gat_sample_metagene_enrichment(gat_ctx* ctx, gat_problem* P, uint32_t seed, int64_t sample_begin, int64_t sample_end,
                                              const uint32_t* feat_start, const uint32_t* feat_end, const uint8_t* feat_minus,
                                              const int64_t* feat_off, int32_t n_tracks, int32_t body_bins, int32_t flank_bins,
                                              int64_t flank_bin_size, int mode, const int64_t* obs_host, int64_t* out_host, gat_stats* stats) {
  const char* who = "gat_sample_metagene_enrichment";
  if (!ctx || !P || !feat_off) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if (int rc = check_sample_range(ctx, sample_begin, sample_end)) return rc;
  MetageneCall T = {who, feat_start, feat_end, feat_minus, feat_off, n_tracks, body_bins, flank_bins, flank_bin_size, mode};
  int rc;
  if ((rc = T.check(ctx, P->n_contigs))) return rc;
  const int64_t S = sample_end - sample_begin, cells = (int64_t)n_tracks * T.bins();
  if (cells > 0 && (!obs_host || !out_host)) return set_err(ctx, GAT_ERR_ARG, "%s: NULL argument", who);
  if ((rc = T.check_words(ctx, S, obs_host, cells))) return rc;
  if ((rc = check_sampled_lists_normalized(ctx, who, P, "the metagene needs normalized lists"))) return rc;
  return fold_over_sampled_batches(ctx, P, stats, seed, sample_begin, S, T, obs_host, cells, out_host);
}
