// tehmm_segment_host.inc -- host side of the kernels in tehmm_segment.hip.h (included by tehmm_hip.hip): the cut
// rows of unsegmented track tables, and the text writer of the segment BED.

namespace {

struct SegCounters {
  int64_t stripes = 0, rewalked = 0;
  std::vector<std::pair<const char *, double>> timing;      // device passes of the last call, milliseconds
};
thread_local SegCounters t_seg;

// events on the null stream between the passes; entry i is the time from mark i - 1 to mark i
struct SegClock {
  std::vector<std::pair<const char *, hipEvent_t>> marks;
  ~SegClock() {
    for (auto &m : marks) (void)hipEventDestroy(m.second);
  }
  hipError_t mark(const char *name) {
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    marks.emplace_back(name, e);
    return hipEventRecord(e, 0);
  }
  hipError_t finish(std::vector<std::pair<const char *, double>> &out) {
    for (size_t i = 1; i < marks.size(); ++i) {
      float ms = 0.f;
      hipError_t rc = hipEventElapsedTime(&ms, marks[i - 1].second, marks[i].second);
      if (rc != hipSuccess) return rc;
      out.emplace_back(marks[i].first, (double)ms);
    }
    return hipSuccess;
  }
};

template <bool PREV>
int seg_chain_passes(const SegParams &sp, int n_tables, const int64_t *table_offsets, int64_t total, uint8_t *d_flag,
                     SegClock &clk) {
  constexpr int64_t S = TEHMM_SEG_STRIPE;
  std::vector<int64_t> st_begin, tbl_stripe0((size_t)n_tables + 1);
  std::vector<uint8_t> st_first;
  st_begin.reserve((size_t)(total / S + n_tables + 1));
  st_first.reserve(st_begin.capacity());
  for (int t = 0; t < n_tables; ++t) {
    tbl_stripe0[(size_t)t] = (int64_t)st_begin.size();
    for (int64_t a = table_offsets[t]; a < table_offsets[t + 1]; a += S) {
      st_begin.push_back(a);
      st_first.push_back(a == table_offsets[t] ? 1 : 0);
    }
  }
  const int64_t ns = (int64_t)st_begin.size();
  tbl_stripe0[(size_t)n_tables] = ns;
  st_begin.push_back(total);
  if ((ns + 3) / 4 > INT_MAX) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_segment_offsets_u8: too many stripes");
  t_seg.stripes = ns;
  DBuf<int64_t> d_sb, d_ts, d_exit, d_meet, d_lexit;
  DBuf<uint8_t> d_sf, d_spec;
  DBuf<unsigned long long> d_cnt;
  HIPCHK(d_sb.upload(st_begin.data(), st_begin.size()));
  HIPCHK(d_sf.upload(st_first.data(), st_first.size()));
  HIPCHK(d_exit.alloc((size_t)ns));
  HIPCHK(d_meet.alloc((size_t)ns));
  HIPCHK(d_lexit.alloc((size_t)ns));
  HIPCHK(d_spec.alloc((size_t)total));
  HIPCHK(d_cnt.alloc(2));
  HIPCHK(hipMemsetAsync(d_spec.p, 0, (size_t)total, 0));
  HIPCHK(hipMemsetAsync(d_flag, 0, (size_t)total, 0));
  HIPCHK(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), 0));
  const dim3 grid((unsigned)((ns + 3) / 4)), block(256);
  hipLaunchKernelGGL((k_seg_spec<PREV>), grid, block, 0, 0, sp, ns, (const int64_t *)d_sb.p, d_spec.p, d_exit.p);
  HIPCHK(clk.mark("speculate"));
  hipLaunchKernelGGL((k_seg_link<PREV>), grid, block, 0, 0, sp, ns, (const int64_t *)d_sb.p, (const uint8_t *)d_sf.p,
                     (const uint8_t *)d_spec.p, (const int64_t *)d_exit.p, d_flag, d_meet.p, d_lexit.p, d_cnt.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("link"));
  unsigned long long cnt[2] = {0, 0};
  HIPCHK(hipMemcpy(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
  if (cnt[0] > 0) {      // marked stripes: the exact walk, one wave per table
    HIPCHK(d_ts.upload(tbl_stripe0.data(), tbl_stripe0.size()));
    hipLaunchKernelGGL((k_seg_rewalk<PREV>), dim3((unsigned)((n_tables + 3) / 4)), block, 0, 0, sp, (int64_t)n_tables,
                       (const int64_t *)d_ts.p, (const int64_t *)d_sb.p, (const uint8_t *)d_spec.p, d_flag, d_meet.p,
                       (const int64_t *)d_lexit.p, d_cnt.p + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("rewalk"));
    HIPCHK(hipMemcpy(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
    t_seg.rewalked = (int64_t)cnt[1];
  }
  hipLaunchKernelGGL(k_seg_merge, grid, block, 0, 0, ns, (const int64_t *)d_sb.p, (const int64_t *)d_meet.p,
                     (const uint8_t *)d_spec.p, d_flag);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("merge"));
  HIPCHK(hipDeviceSynchronize());      // the buffers above go back to the pool
  return TEHMM_OK;
}

}  // namespace

int64_t tehmm_segment_stripe_rows(void) { return TEHMM_SEG_STRIPE; }

int tehmm_segment_last_counters(int64_t *stripes, int64_t *stripes_rewalked) {
  if (stripes) *stripes = t_seg.stripes;
  if (stripes_rewalked) *stripes_rewalked = t_seg.rewalked;
  return TEHMM_OK;
}

int tehmm_segment_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_segment_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_seg.timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_segment_offsets_u8(int n_tables, const int64_t *table_offsets, int K, const uint8_t *data,
                             const uint8_t *ignore, const uint8_t *cut, int thresh, int comp_prev, int64_t maxLen,
                             int64_t fixLen, int64_t cap, int64_t *cuts, int64_t *n_cuts, int64_t *n_total,
                             uint64_t *stats_hist) {
  t_seg = SegCounters();
  if (n_tables <= 0 || !table_offsets || K <= 0 || !data || !ignore || !cut || cap < 0 || (cap > 0 && !cuts) ||
      !n_cuts || !n_total)
    return fail(TEHMM_ERR_ARG, "tehmm_segment_offsets_u8: bad argument");
  if (K > TEHMM_MAX_TRACKS) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_segment_offsets_u8: more than 128 tracks");
  if (thresh < 0) return fail(TEHMM_ERR_ARG, "tehmm_segment_offsets_u8: negative thresh");
  if (table_offsets[0] != 0) return fail(TEHMM_ERR_ARG, "tehmm_segment_offsets_u8: table_offsets must start at 0");
  for (int t = 0; t < n_tables; ++t)
    if (table_offsets[t + 1] <= table_offsets[t])
      return fail(TEHMM_ERR_ARG, "tehmm_segment_offsets_u8: table_offsets must ascend, with no empty table");
  const int64_t total = table_offsets[n_tables];
  if (total > 0x7fffffffll)
    return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_segment_offsets_u8: more than 2^31 - 1 rows in one call");
  // a limit no segment can reach is no limit (and L + maxLen stays far from overflow)
  if (maxLen < 0 || maxLen >= total) maxLen = 0;
  if (fixLen < 0) fixLen = 0;
  const bool fixed = fixLen > 0, prev = comp_prev != 0;
  const int KW = (K + 3) / 4;

  SegClock clk;
  DBuf<uint8_t> d_data, d_ign, d_flag;
  DBuf<uint32_t> d_packed, d_cutw;
  DBuf<int64_t> d_off, d_row, d_rel, d_rank;
  DBuf<unsigned> d_blk;
  DBuf<int64_t> d_tot;
  DBuf<unsigned long long> d_hist;
  const dim3 block(256);
  HIPCHK(clk.mark("start"));
  HIPCHK(d_off.upload(table_offsets, (size_t)n_tables + 1));
  HIPCHK(d_flag.alloc((size_t)total));
  SegParams sp;
  sp.packed = nullptr;
  sp.cutw = nullptr;
  sp.KW = KW;
  sp.thresh = thresh;
  sp.maxLen = maxLen;
  if (fixed) {
    hipLaunchKernelGGL(k_seg_fixlen, dim3(grid_for(total, 256, 1 << 16)), block, 0, 0, total, (int64_t)n_tables,
                       (const int64_t *)d_off.p, fixLen, d_flag.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("fixlen"));
  } else {
    std::vector<uint32_t> cutw((size_t)KW, 0u);
    for (int k = 0; k < K; ++k)
      if (cut[k] != 0 && ignore[k] == 0) cutw[(size_t)k / 4] |= 0xffu << (8 * (k % 4));
    HIPCHK(d_data.upload(data, (size_t)total * K));
    HIPCHK(d_ign.upload(ignore, (size_t)K));
    HIPCHK(d_cutw.upload(cutw.data(), cutw.size()));
    HIPCHK(clk.mark("upload"));
    HIPCHK(d_packed.alloc((size_t)total * KW));
    hipLaunchKernelGGL(k_seg_pack, dim3(grid_for(total * KW, 256, 1 << 16)), block, 0, 0, total, K, KW,
                       (const uint8_t *)d_data.p, (const uint8_t *)d_ign.p, d_packed.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("pack"));
    sp.packed = d_packed.p;
    sp.cutw = d_cutw.p;
    if (prev && maxLen == 0) {
      hipLaunchKernelGGL(k_seg_prev_flags, dim3(grid_for(total, 256, 1 << 16)), block, 0, 0, sp, total, d_flag.p);
      hipLaunchKernelGGL(k_seg_mark_starts, dim3(grid_for(n_tables, 256, INT_MAX)), block, 0, 0, (int64_t)n_tables,
                         (const int64_t *)d_off.p, d_flag.p);
      HIPCHK(hipGetLastError());
      HIPCHK(clk.mark("flags"));
    } else {
      const int rc = prev ? seg_chain_passes<true>(sp, n_tables, table_offsets, total, d_flag.p, clk)
                          : seg_chain_passes<false>(sp, n_tables, table_offsets, total, d_flag.p, clk);
      if (rc) return rc;
    }
  }
  // compaction: flags -> ascending rows
  const int64_t nb = (total + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_tot.alloc(1));
  hipLaunchKernelGGL(k_seg_count, dim3((unsigned)nb), block, 0, 0, total, (const uint8_t *)d_flag.p, d_blk.p);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), block, 0, 0, nb, d_blk.p, d_tot.p);
  HIPCHK(hipGetLastError());
  int64_t nt = 0;
  HIPCHK(hipMemcpy(&nt, d_tot.p, sizeof(nt), hipMemcpyDeviceToHost));
  if (nt < n_tables || nt > total) return fail(TEHMM_ERR_HIP, "tehmm_segment_offsets_u8: inconsistent cut count");
  HIPCHK(d_row.alloc((size_t)nt));
  HIPCHK(d_rel.alloc((size_t)nt));
  HIPCHK(d_rank.alloc((size_t)n_tables));
  hipLaunchKernelGGL(k_seg_scatter, dim3((unsigned)nb), block, 0, 0, total, (const uint8_t *)d_flag.p,
                     (const unsigned *)d_blk.p, (int64_t)n_tables, (const int64_t *)d_off.p, d_row.p, d_rel.p,
                     d_rank.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("compact"));
  std::vector<int64_t> rank((size_t)n_tables);
  HIPCHK(hipMemcpy(rank.data(), d_rank.p, rank.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int t = 0; t < n_tables; ++t) n_cuts[t] = (t + 1 < n_tables ? rank[(size_t)t + 1] : nt) - rank[(size_t)t];
  *n_total = nt;
  if (stats_hist) {
    const size_t hn = (size_t)K * (size_t)(K + 1);
    HIPCHK(d_hist.alloc(hn));
    HIPCHK(hipMemset(d_hist.p, 0, hn * sizeof(unsigned long long)));
    if (!fixed) {
      hipLaunchKernelGGL(k_seg_stats, dim3(grid_for(nt, 256, 1 << 16)), block, 0, 0, sp, K, prev ? 1 : 0, nt,
                         (const int64_t *)d_row.p, (const int64_t *)d_rel.p, d_hist.p);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(clk.mark("stats"));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram cell");
    HIPCHK(hipMemcpy(stats_hist, d_hist.p, hn * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  if (nt <= cap && nt > 0) HIPCHK(hipMemcpy(cuts, d_rel.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_seg.timing));
  return TEHMM_OK;
}

// Host-side writer of the segment BED (segmentTracks.py:222-236): "chrom\tstart\tend\t<label>\n" with label
// hex(first_label + i)[2:], i.e. lower-case hexadecimal without a prefix.
int tehmm_write_segments_bed(const char *path, int append, const char *chrom, int64_t n, const int64_t *starts,
                             const int64_t *ends, int64_t first_label) {
  if (!path || !chrom || n < 0 || (n > 0 && (!starts || !ends)) || first_label < 0)
    return fail(TEHMM_ERR_ARG, "tehmm_write_segments_bed: bad argument");
  FILE *f = std::fopen(path, append ? "a" : "w");
  if (!f) return fail(TEHMM_ERR_ARG, std::string("tehmm_write_segments_bed: cannot open ") + path);
  std::string buf;
  buf.reserve(1 << 22);
  char num[96];
  const size_t clen = std::strlen(chrom);
  int rc = TEHMM_OK;
  for (int64_t i = 0; i < n && rc == TEHMM_OK; ++i) {
    buf.append(chrom, clen);
    const int k = std::snprintf(num, sizeof(num), "\t%lld\t%lld\t%llx\n", (long long)starts[i], (long long)ends[i],
                                (unsigned long long)(first_label + i));
    buf.append(num, (size_t)k);
    if (buf.size() > (1u << 22) - 256) {
      if (std::fwrite(buf.data(), 1, buf.size(), f) != buf.size())
        rc = fail(TEHMM_ERR_ARG, "tehmm_write_segments_bed: write failed");
      buf.clear();
    }
  }
  if (rc == TEHMM_OK && !buf.empty() && std::fwrite(buf.data(), 1, buf.size(), f) != buf.size())
    rc = fail(TEHMM_ERR_ARG, "tehmm_write_segments_bed: write failed");
  if (std::fclose(f) != 0 && rc == TEHMM_OK) rc = fail(TEHMM_ERR_ARG, "tehmm_write_segments_bed: close failed");
  return rc;
}
