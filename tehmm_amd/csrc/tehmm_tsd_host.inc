// tehmm_tsd_host.inc -- host side of the kernels in tehmm_tsd.hip.h (included by tehmm_hip.hip, behind
// tehmm_segment_host.inc whose SegClock it uses): the TSD finder and the overlap clean-up.

namespace {

thread_local std::vector<std::pair<const char *, double>> t_tsd_timing;      // device passes of the last call

}  // namespace

int tehmm_tsd_window(void) { return TEHMM_TSD_WINDOW; }

int tehmm_tsd_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_tsd_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_tsd_timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_tsd_find(int n_seq, const uint8_t *bases, const int64_t *seq_offsets, int64_t n, const int32_t *seq_index,
                   const int64_t *start, const int64_t *end, int min_len, int max_len, int left, int right, int overlap,
                   int max_score, int all, int32_t *counts, int64_t cap, int64_t *left_start, int64_t *left_end,
                   int64_t *d1, int64_t *right_start, int64_t *right_end, int64_t *d2, int64_t *n_out) {
  const std::string who = "tehmm_tsd_find";
  t_tsd_timing.clear();
  if (!n_out) return fail(TEHMM_ERR_ARG, who + ": NULL n_out");
  *n_out = 0;
  if (!bases || !seq_offsets || !seq_index || !start || !end || !counts) return fail(TEHMM_ERR_ARG, who + ": NULL argument");
  if (cap < 0 || (cap > 0 && (!left_start || !left_end || !d1 || !right_start || !right_end || !d2)))
    return fail(TEHMM_ERR_ARG, who + ": cap < 0, or a NULL column with cap > 0");
  if (n_seq < 1) return fail(TEHMM_ERR_ARG, who + ": n_seq < 1");
  if (n < 1) return fail(TEHMM_ERR_ARG, who + ": n < 1");
  if (min_len < 1) return fail(TEHMM_ERR_ARG, who + ": min < 1");
  if (min_len > max_len) return fail(TEHMM_ERR_ARG, who + ": min > max");
  if (min_len > TEHMM_TSD_MAX_K) return fail(TEHMM_ERR_ARG, who + ": min > 21 (the reference's k-mer hash stops there)");
  if (n > 0x7fffffffll) return fail(TEHMM_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 elements");
  const int ov = overlap > 0 ? overlap : 0;      // (a negative overlap searches what overlap 0 does)
  if ((int64_t)left + ov - 1 > TEHMM_TSD_WINDOW || (int64_t)right + ov - 1 > TEHMM_TSD_WINDOW)
    return fail(TEHMM_ERR_UNSUPPORTED, who + ": a search window (left + overlap - 1, right + overlap - 1) above 64 bases");
  if (seq_offsets[0] < 0) return fail(TEHMM_ERR_ARG, who + ": seq_offsets[0] < 0");
  for (int q = 0; q < n_seq; ++q)
    if (seq_offsets[q + 1] < seq_offsets[q])
      return fail(TEHMM_ERR_ARG, who + ": seq_offsets decrease at sequence " + std::to_string(q));
  for (int64_t i = 0; i < n; ++i) {
    const char *what = seq_index[i] < 0 || seq_index[i] >= n_seq ? "has a seq_index out of range"
                       : start[i] < 0                            ? "has start < 0"
                       : start[i] > end[i]                       ? "has start > end"
                                                                 : nullptr;
    if (what) return fail(TEHMM_ERR_ARG, who + ": element " + std::to_string((long long)i) + " " + what);
  }
  TsdOpt o;
  o.k = min_len;
  o.left = left;
  o.right = right;
  o.overlap = ov;
  const int64_t P = std::max<int64_t>(min_len, (int64_t)max_len - min_len);
  o.per = (int)std::min<int64_t>(P - min_len + 1, TEHMM_TSD_WINDOW);
  o.max_score = max_score < -1 ? -2 : max_score;
  o.all = all ? 1 : 0;

  SegClock clk;
  const size_t total = (size_t)seq_offsets[n_seq], padded = (total + 15) / 8 * 8;
  DBuf<uint8_t> d_bases;
  DBuf<int64_t> d_so, d_start, d_end, d_blk, d_tot, d_off;
  DBuf<int32_t> d_si, d_count;
  DBuf<uint32_t> d_best;
  DBuf<unsigned long long> d_viol;
  HIPCHK(clk.mark("start"));
  HIPCHK(d_bases.alloc(padded));
  const size_t tail = padded >= 16 ? padded - 16 : 0;      // the pad behind the last base reads as zeros
  HIPCHK(hipMemsetAsync(d_bases.p + tail, 0, padded - tail, 0));
  if (total) HIPCHK(hipMemcpy(d_bases.p, bases, total, hipMemcpyHostToDevice));
  HIPCHK(d_so.upload(seq_offsets, (size_t)n_seq + 1));
  HIPCHK(d_si.upload(seq_index, (size_t)n));
  HIPCHK(d_start.upload(start, (size_t)n));
  HIPCHK(d_end.upload(end, (size_t)n));
  HIPCHK(clk.mark("upload"));
  const int64_t nb = (n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  HIPCHK(d_count.alloc((size_t)n));
  HIPCHK(d_best.alloc((size_t)n));
  HIPCHK(d_off.alloc((size_t)n));
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_tot.alloc(1));
  HIPCHK(d_viol.alloc(1));
  HIPCHK(hipMemsetAsync(d_viol.p, 0xff, sizeof(unsigned long long), 0));
  TsdElems el;
  el.n = n;
  el.seq = d_si.p;
  el.start = d_start.p;
  el.end = d_end.p;
  el.seq_off = d_so.p;
  el.bases = d_bases.p;
  const dim3 block(256), grid(grid_for(n, 256, 1 << 16));
  hipLaunchKernelGGL(k_tsd_find, grid, block, 0, 0, el, o, d_count.p, d_best.p, d_viol.p);
  HIPCHK(hipGetLastError());
  unsigned long long viol = 0;
  HIPCHK(hipMemcpy(&viol, d_viol.p, sizeof(viol), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("find"));
  if (viol != ~0ull)
    return fail(TEHMM_ERR_ARG, who + ": element " + std::to_string(viol) +
                                   " has a base other than ACGTNacgtn in a search window");
  hipLaunchKernelGGL(k_tsd_blocksum, dim3((unsigned)nb), block, 0, 0, n, (const int32_t *)d_count.p, d_blk.p);
  hipLaunchKernelGGL(k_tsd_scan_blocks, dim3(1), block, 0, 0, nb, d_blk.p, d_tot.p);
  hipLaunchKernelGGL(k_tsd_offsets, dim3((unsigned)nb), block, 0, 0, n, (const int32_t *)d_count.p,
                     (const int64_t *)d_blk.p, d_off.p);
  HIPCHK(hipGetLastError());
  int64_t nt = 0;
  HIPCHK(hipMemcpy(&nt, d_tot.p, sizeof(nt), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("scan"));
  if (nt < 0 || nt > n * (int64_t)(TEHMM_TSD_WINDOW * TEHMM_TSD_WINDOW))
    return fail(TEHMM_ERR_HIP, who + ": inconsistent match count");
  const int64_t nw = nt < cap ? nt : cap;
  DBuf<int64_t> d_col[6];
  int64_t *host_col[6] = {left_start, left_end, d1, right_start, right_end, d2};
  if (nw > 0) {
    for (auto &c : d_col) HIPCHK(c.alloc((size_t)nw));
    TsdOut out;
    out.cap = nw;
    out.ls = d_col[0].p;
    out.le = d_col[1].p;
    out.d1 = d_col[2].p;
    out.rs = d_col[3].p;
    out.re = d_col[4].p;
    out.d2 = d_col[5].p;
    if (o.all)
      hipLaunchKernelGGL((k_tsd_scatter<true>), grid, block, 0, 0, el, o, (const int32_t *)d_count.p,
                         (const uint32_t *)d_best.p, (const int64_t *)d_off.p, out);
    else
      hipLaunchKernelGGL((k_tsd_scatter<false>), grid, block, 0, 0, el, o, (const int32_t *)d_count.p,
                         (const uint32_t *)d_best.p, (const int64_t *)d_off.p, out);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("scatter"));
  }
  HIPCHK(hipMemcpy(counts, d_count.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int q = 0; q < 6 && nw > 0; ++q)
    HIPCHK(hipMemcpy(host_col[q], d_col[q].p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_tsd_timing));
  *n_out = nt;
  return TEHMM_OK;
}

int tehmm_remove_overlaps(int64_t n, const int32_t *chrom_id, const int64_t *start, const int64_t *end, int64_t cap,
                          int64_t *out_index, int64_t *out_start, int64_t *n_out) {
  const std::string who = "tehmm_remove_overlaps";
  t_tsd_timing.clear();
  if (!n_out) return fail(TEHMM_ERR_ARG, who + ": NULL n_out");
  *n_out = 0;
  if (!chrom_id || !start || !end) return fail(TEHMM_ERR_ARG, who + ": NULL list");
  if (cap < 0 || (cap > 0 && (!out_index || !out_start)))
    return fail(TEHMM_ERR_ARG, who + ": cap < 0, or a NULL output with cap > 0");
  if (n < 1) return fail(TEHMM_ERR_ARG, who + ": a list holds at least one interval");
  if (n > 0x7fffffffll) return fail(TEHMM_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 intervals");
  SegClock clk;
  DBuf<int32_t> d_chrom, d_aggc;
  DBuf<int64_t> d_start, d_end, d_aggm, d_ns, d_tot, d_oi, d_os;
  DBuf<uint8_t> d_keep;
  DBuf<unsigned> d_blk;
  DBuf<unsigned long long> d_viol;
  HIPCHK(clk.mark("start"));
  HIPCHK(d_chrom.upload(chrom_id, (size_t)n));
  HIPCHK(d_start.upload(start, (size_t)n));
  HIPCHK(d_end.upload(end, (size_t)n));
  HIPCHK(clk.mark("upload"));
  const int64_t nb = (n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  HIPCHK(d_viol.alloc(1));
  HIPCHK(hipMemsetAsync(d_viol.p, 0xff, sizeof(unsigned long long), 0));
  const dim3 block(256), blocks((unsigned)nb);
  hipLaunchKernelGGL(k_rmo_check, dim3(grid_for(n, 256, 1 << 16)), block, 0, 0, n, (const int32_t *)d_chrom.p,
                     (const int64_t *)d_start.p, d_viol.p);
  HIPCHK(hipGetLastError());
  unsigned long long viol = 0;
  HIPCHK(hipMemcpy(&viol, d_viol.p, sizeof(viol), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("check"));
  if (viol != ~0ull)
    return fail(TEHMM_ERR_ARG, who + ": interval " + std::to_string(viol) +
                                   " lies before its predecessor: the list is not sorted by (chrom id, start)");
  HIPCHK(d_aggc.alloc((size_t)nb));
  HIPCHK(d_aggm.alloc((size_t)nb));
  HIPCHK(d_ns.alloc((size_t)n));
  HIPCHK(d_keep.alloc((size_t)n));
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_tot.alloc(1));
  hipLaunchKernelGGL(k_rmo_blockagg, blocks, block, 0, 0, n, (const int32_t *)d_chrom.p, (const int64_t *)d_end.p,
                     d_aggc.p, d_aggm.p);
  hipLaunchKernelGGL(k_rmo_scan_blocks, dim3(1), block, 0, 0, nb, d_aggc.p, d_aggm.p);
  hipLaunchKernelGGL(k_rmo_apply, blocks, block, 0, 0, n, (const int32_t *)d_chrom.p, (const int64_t *)d_start.p,
                     (const int64_t *)d_end.p, (const int32_t *)d_aggc.p, (const int64_t *)d_aggm.p, d_ns.p, d_keep.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("running_max"));
  hipLaunchKernelGGL(k_seg_count, blocks, block, 0, 0, n, (const uint8_t *)d_keep.p, d_blk.p);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), block, 0, 0, nb, d_blk.p, d_tot.p);
  HIPCHK(hipGetLastError());
  int64_t nt = 0;
  HIPCHK(hipMemcpy(&nt, d_tot.p, sizeof(nt), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("count"));
  if (nt < 0 || nt > n) return fail(TEHMM_ERR_HIP, who + ": inconsistent count");
  const int64_t nw = nt < cap ? nt : cap;
  if (nw > 0) {
    HIPCHK(d_oi.alloc((size_t)nw));
    HIPCHK(d_os.alloc((size_t)nw));
    hipLaunchKernelGGL(k_rmo_scatter, blocks, block, 0, 0, n, (const uint8_t *)d_keep.p, (const unsigned *)d_blk.p,
                       (const int64_t *)d_ns.p, nw, d_oi.p, d_os.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("scatter"));
    HIPCHK(hipMemcpy(out_index, d_oi.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_start, d_os.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(clk.mark("download"));
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_tsd_timing));
  *n_out = nt;
  return TEHMM_OK;
}
