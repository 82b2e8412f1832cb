// tehmm_masking_host.inc -- host side of the kernels in tehmm_masking.hip.h (included by tehmm_hip.hip, behind
// tehmm_segment_host.inc whose SegClock it uses): merge, subtract, intersect and the mask fill.

namespace {

thread_local std::vector<std::pair<const char *, double>> t_msk_timing;      // device passes of the last call

struct MskList {
  DBuf<int32_t> chrom;
  DBuf<int64_t> start, end;
  MskView view;
};

int msk_upload(MskList &l, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end) {
  HIPCHK(l.chrom.upload(chrom, (size_t)n));
  HIPCHK(l.start.upload(start, (size_t)n));
  HIPCHK(l.end.upload(end, (size_t)n));
  l.view.n = n;
  l.view.chrom = l.chrom.p;
  l.view.start = l.start.p;
  l.view.end = l.end.p;
  return TEHMM_OK;
}

// the pre-device checks every list gets
int msk_list_args(const std::string &who, const char *list, int64_t n, const void *chrom, const void *start,
                  const void *end) {
  if (!chrom || !start || !end) return fail(TEHMM_ERR_ARG, who + ": NULL column of " + list);
  if (n < 1) return fail(TEHMM_ERR_ARG, who + ": " + list + " holds no interval (n < 1)");
  if (n > 0x7fffffffll) return fail(TEHMM_ERR_UNSUPPORTED, who + ": " + list + " holds more than 2^31 - 1 intervals");
  return TEHMM_OK;
}

// start < end and the stated order, on the device; the lowest offender is named
int msk_check(const std::string &who, const char *list, const MskList &l, int order, DBuf<unsigned long long> &d_viol) {
  HIPCHK(d_viol.alloc(2));
  HIPCHK(hipMemsetAsync(d_viol.p, 0xff, 2 * sizeof(unsigned long long), 0));
  hipLaunchKernelGGL(k_msk_check, dim3(grid_for(l.view.n, 256, 1 << 16)), dim3(256), 0, 0, l.view, order, d_viol.p);
  HIPCHK(hipGetLastError());
  unsigned long long viol[2] = {0, 0};
  HIPCHK(hipMemcpy(viol, d_viol.p, sizeof(viol), hipMemcpyDeviceToHost));
  if (viol[0] == ~0ull && viol[1] == ~0ull) return TEHMM_OK;
  if (viol[0] <= viol[1])
    return fail(TEHMM_ERR_ARG, who + ": interval " + std::to_string(viol[0]) + " of " + list + " has start >= end");
  const char *what = order == TEHMM_MASK_ORDER_DISJOINT ? "the list is not sorted by (chrom id, start) and disjoint"
                     : order == TEHMM_MASK_ORDER_TRIPLE ? "the list is not sorted by (chrom id, start, end)"
                                                        : "the list is not sorted by (chrom id, start)";
  return fail(TEHMM_ERR_ARG,
              who + ": interval " + std::to_string(viol[1]) + " of " + list + " lies before its predecessor: " + what);
}

// off[i] = sum of count[0 .. i) on the device, *total the sum
int msk_scan(int64_t n, const uint32_t *d_count, DBuf<int64_t> &d_off, int64_t *total) {
  const int64_t nb = (n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  DBuf<int64_t> d_blk, d_tot;
  HIPCHK(d_off.alloc((size_t)n));
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_tot.alloc(1));
  const dim3 block(256), blocks((unsigned)nb);
  hipLaunchKernelGGL(k_msk_blocksum, blocks, block, 0, 0, n, d_count, d_blk.p);
  hipLaunchKernelGGL(k_tsd_scan_blocks, dim3(1), block, 0, 0, nb, d_blk.p, d_tot.p);
  hipLaunchKernelGGL(k_msk_offsets, blocks, block, 0, 0, n, d_count, (const int64_t *)d_blk.p, d_off.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(total, d_tot.p, sizeof(int64_t), hipMemcpyDeviceToHost));
  return TEHMM_OK;
}

// flags -> scanned workgroup counts and the number of set flags
int msk_flag_counts(int64_t n, const uint8_t *d_flag, DBuf<unsigned> &d_blk, int64_t *total) {
  const int64_t nb = (n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  DBuf<int64_t> d_tot;
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_tot.alloc(1));
  hipLaunchKernelGGL(k_seg_count, dim3((unsigned)nb), dim3(256), 0, 0, n, d_flag, d_blk.p);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, 0, nb, d_blk.p, d_tot.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(total, d_tot.p, sizeof(int64_t), hipMemcpyDeviceToHost));
  return TEHMM_OK;
}

template <bool SUB>
int msk_pieces(const std::string &who, int64_t nA, const int32_t *chromA, const int64_t *startA, const int64_t *endA,
               int64_t nB, const int32_t *chromB, const int64_t *startB, const int64_t *endB, int64_t cap,
               int64_t *out_src, int64_t *out_start, int64_t *out_end, int64_t *n_out) {
  t_msk_timing.clear();
  if (!n_out) return fail(TEHMM_ERR_ARG, who + ": NULL n_out");
  *n_out = 0;
  int rc = msk_list_args(who, "A", nA, chromA, startA, endA);
  if (rc == TEHMM_OK) rc = msk_list_args(who, "B", nB, chromB, startB, endB);
  if (rc != TEHMM_OK) return rc;
  if (cap < 0 || (cap > 0 && (!out_src || !out_start || !out_end)))
    return fail(TEHMM_ERR_ARG, who + ": cap < 0, or a NULL column with cap > 0");
  SegClock clk;
  MskList a, b;
  DBuf<unsigned long long> d_viol;
  HIPCHK(clk.mark("start"));
  if ((rc = msk_upload(a, nA, chromA, startA, endA)) != TEHMM_OK) return rc;
  if ((rc = msk_upload(b, nB, chromB, startB, endB)) != TEHMM_OK) return rc;
  HIPCHK(clk.mark("upload"));
  if ((rc = msk_check(who, "A", a, TEHMM_MASK_ORDER_NONE, d_viol)) != TEHMM_OK) return rc;
  if ((rc = msk_check(who, "B", b, TEHMM_MASK_ORDER_DISJOINT, d_viol)) != TEHMM_OK) return rc;
  HIPCHK(clk.mark("check"));
  const dim3 block(256);
  DBuf<uint32_t> d_gap, d_count;
  DBuf<int64_t> d_G, d_off;
  DBuf<int32_t> d_lo, d_hi;
  int64_t n_gaps = 0, nt = 0;
  if (SUB) {
    HIPCHK(d_gap.alloc((size_t)nB + 1));
    hipLaunchKernelGGL(k_msk_gap_flags, dim3(grid_for(nB + 1, 256, 1 << 16)), block, 0, 0, b.view, d_gap.p);
    if ((rc = msk_scan(nB + 1, d_gap.p, d_G, &n_gaps)) != TEHMM_OK) return rc;
    HIPCHK(clk.mark("gaps"));
  }
  HIPCHK(d_count.alloc((size_t)nA));
  HIPCHK(d_lo.alloc((size_t)nA));
  HIPCHK(d_hi.alloc((size_t)nA));
  hipLaunchKernelGGL((k_msk_count<SUB>), dim3(grid_for(nA, 256, 1 << 16)), block, 0, 0, a.view, b.view,
                     (const int64_t *)d_G.p, d_count.p, d_lo.p, d_hi.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("count"));
  if ((rc = msk_scan(nA, d_count.p, d_off, &nt)) != TEHMM_OK) return rc;
  HIPCHK(clk.mark("scan"));
  if (nt < 0) return fail(TEHMM_ERR_HIP, who + ": inconsistent piece count");
  const int64_t nw = nt < cap ? nt : cap;
  if (nw > 0) {
    DBuf<int64_t> d_src, d_os, d_oe;
    HIPCHK(d_src.alloc((size_t)nw));
    HIPCHK(d_os.alloc((size_t)nw));
    HIPCHK(d_oe.alloc((size_t)nw));
    hipLaunchKernelGGL((k_msk_emit<SUB>), dim3(grid_for(nw, 256, 1 << 16)), block, 0, 0, nw, a.view, b.view,
                       (const int64_t *)d_G.p, (const int64_t *)d_off.p, (const int32_t *)d_lo.p,
                       (const int32_t *)d_hi.p, d_src.p, d_os.p, d_oe.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("emit"));
    HIPCHK(hipMemcpy(out_src, d_src.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_start, d_os.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_end, d_oe.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(clk.mark("download"));
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_msk_timing));
  *n_out = nt;
  return TEHMM_OK;
}

}  // namespace

int tehmm_masking_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_masking_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_msk_timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_intervals_merge(int64_t n, const int32_t *chrom_id, const int64_t *start, const int64_t *end, int64_t min_len,
                          int64_t max_len, int64_t cap, int32_t *out_chrom, int64_t *out_start, int64_t *out_end,
                          int64_t *n_out) {
  const std::string who = "tehmm_intervals_merge";
  t_msk_timing.clear();
  if (!n_out) return fail(TEHMM_ERR_ARG, who + ": NULL n_out");
  *n_out = 0;
  int rc = msk_list_args(who, "the list", n, chrom_id, start, end);
  if (rc != TEHMM_OK) return rc;
  if (cap < 0 || (cap > 0 && (!out_chrom || !out_start || !out_end)))
    return fail(TEHMM_ERR_ARG, who + ": cap < 0, or a NULL column with cap > 0");
  SegClock clk;
  MskList l;
  DBuf<unsigned long long> d_viol;
  HIPCHK(clk.mark("start"));
  if ((rc = msk_upload(l, n, chrom_id, start, end)) != TEHMM_OK) return rc;
  HIPCHK(clk.mark("upload"));
  if ((rc = msk_check(who, "the list", l, TEHMM_MASK_ORDER_SORTED, d_viol)) != TEHMM_OK) return rc;
  HIPCHK(clk.mark("check"));
  const int64_t nb = (n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  const dim3 block(256), blocks((unsigned)nb);
  DBuf<int32_t> d_aggc, d_rc, d_oc;
  DBuf<int64_t> d_aggm, d_rmax, d_rs, d_re, d_os, d_oe;
  DBuf<uint8_t> d_head, d_keep;
  DBuf<unsigned> d_blk, d_blk2;
  HIPCHK(d_aggc.alloc((size_t)nb));
  HIPCHK(d_aggm.alloc((size_t)nb));
  HIPCHK(d_head.alloc((size_t)n));
  HIPCHK(d_rmax.alloc((size_t)n));
  hipLaunchKernelGGL(k_rmo_blockagg, blocks, block, 0, 0, n, l.view.chrom, l.view.end, d_aggc.p, d_aggm.p);
  hipLaunchKernelGGL(k_rmo_scan_blocks, dim3(1), block, 0, 0, nb, d_aggc.p, d_aggm.p);
  hipLaunchKernelGGL(k_msk_merge_apply, blocks, block, 0, 0, n, l.view.chrom, l.view.start, l.view.end,
                     (const int32_t *)d_aggc.p, (const int64_t *)d_aggm.p, d_head.p, d_rmax.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("running_max"));
  int64_t nr = 0, nt = 0;
  if ((rc = msk_flag_counts(n, d_head.p, d_blk, &nr)) != TEHMM_OK) return rc;
  if (nr < 1 || nr > n) return fail(TEHMM_ERR_HIP, who + ": inconsistent run count");
  HIPCHK(d_rc.alloc((size_t)nr));
  HIPCHK(d_rs.alloc((size_t)nr));
  HIPCHK(d_re.alloc((size_t)nr));
  HIPCHK(d_keep.alloc((size_t)nr));
  hipLaunchKernelGGL(k_msk_merge_runs, blocks, block, 0, 0, n, (const uint8_t *)d_head.p, (const unsigned *)d_blk.p,
                     l.view.chrom, l.view.start, (const int64_t *)d_rmax.p, d_rc.p, d_rs.p, d_re.p);
  hipLaunchKernelGGL(k_msk_len_flags, dim3(grid_for(nr, 256, 1 << 16)), block, 0, 0, nr, (const int64_t *)d_rs.p,
                     (const int64_t *)d_re.p, min_len, max_len, d_keep.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("runs"));
  if ((rc = msk_flag_counts(nr, d_keep.p, d_blk2, &nt)) != TEHMM_OK) return rc;
  if (nt < 0 || nt > nr) return fail(TEHMM_ERR_HIP, who + ": inconsistent count");
  HIPCHK(clk.mark("filter"));
  const int64_t nw = nt < cap ? nt : cap;
  if (nw > 0) {
    const int64_t nrb = (nr + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
    HIPCHK(d_oc.alloc((size_t)nw));
    HIPCHK(d_os.alloc((size_t)nw));
    HIPCHK(d_oe.alloc((size_t)nw));
    hipLaunchKernelGGL(k_msk_compact, dim3((unsigned)nrb), block, 0, 0, nr, (const uint8_t *)d_keep.p,
                       (const unsigned *)d_blk2.p, (const int32_t *)d_rc.p, (const int64_t *)d_rs.p,
                       (const int64_t *)d_re.p, nw, d_oc.p, d_os.p, d_oe.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("scatter"));
    HIPCHK(hipMemcpy(out_chrom, d_oc.p, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_start, d_os.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_end, d_oe.p, (size_t)nw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(clk.mark("download"));
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_msk_timing));
  *n_out = nt;
  return TEHMM_OK;
}

int tehmm_intervals_subtract(int64_t nA, const int32_t *chromA, const int64_t *startA, const int64_t *endA, int64_t nB,
                             const int32_t *chromB, const int64_t *startB, const int64_t *endB, int64_t cap,
                             int64_t *out_src, int64_t *out_start, int64_t *out_end, int64_t *n_out) {
  return msk_pieces<true>("tehmm_intervals_subtract", nA, chromA, startA, endA, nB, chromB, startB, endB, cap, out_src,
                          out_start, out_end, n_out);
}

int tehmm_intervals_intersect(int64_t nA, const int32_t *chromA, const int64_t *startA, const int64_t *endA, int64_t nB,
                              const int32_t *chromB, const int64_t *startB, const int64_t *endB, int64_t cap,
                              int64_t *out_src, int64_t *out_start, int64_t *out_end, int64_t *n_out) {
  return msk_pieces<false>("tehmm_intervals_intersect", nA, chromA, startA, endA, nB, chromB, startB, endB, cap, out_src,
                           out_start, out_end, n_out);
}

int tehmm_mask_fill(int64_t nM, const int32_t *chromM, const int64_t *startM, const int64_t *endM, int64_t nI,
                    const int32_t *chromI, const int64_t *startI, const int64_t *endI, const int32_t *labelI, int L,
                    const uint8_t *two_sided, const uint8_t *one_sided, int only_default, int64_t max_len,
                    int32_t *out_label) {
  const std::string who = "tehmm_mask_fill";
  t_msk_timing.clear();
  int rc = msk_list_args(who, "the masks", nM, chromM, startM, endM);
  if (rc == TEHMM_OK) rc = msk_list_args(who, "the prediction", nI, chromI, startI, endI);
  if (rc != TEHMM_OK) return rc;
  if (!labelI || !out_label) return fail(TEHMM_ERR_ARG, who + ": NULL labels");
  if (L < 1) return fail(TEHMM_ERR_ARG, who + ": L < 1");
  if (L > TEHMM_MASK_MAX_LABELS) return fail(TEHMM_ERR_UNSUPPORTED, who + ": more than 2048 labels");
  std::vector<uint8_t> two((size_t)L, 1), one((size_t)L, 0);
  for (int k = 0; k < L; ++k) {
    if (two_sided) two[(size_t)k] = two_sided[k] ? 1 : 0;
    if (one_sided) one[(size_t)k] = one_sided[k] ? 1 : 0;
  }
  SegClock clk;
  MskList m, iv;
  DBuf<int32_t> d_label, d_out;
  DBuf<uint8_t> d_two, d_one;
  DBuf<unsigned long long> d_viol, d_v2;
  HIPCHK(clk.mark("start"));
  if ((rc = msk_upload(m, nM, chromM, startM, endM)) != TEHMM_OK) return rc;
  if ((rc = msk_upload(iv, nI, chromI, startI, endI)) != TEHMM_OK) return rc;
  HIPCHK(d_label.upload(labelI, (size_t)nI));
  HIPCHK(d_two.upload(two.data(), (size_t)L));
  HIPCHK(d_one.upload(one.data(), (size_t)L));
  HIPCHK(clk.mark("upload"));
  if ((rc = msk_check(who, "the masks", m, TEHMM_MASK_ORDER_DISJOINT, d_viol)) != TEHMM_OK) return rc;
  if ((rc = msk_check(who, "the prediction", iv, TEHMM_MASK_ORDER_TRIPLE, d_viol)) != TEHMM_OK) return rc;
  const dim3 block(256);
  unsigned long long viol = 0;
  HIPCHK(d_v2.alloc(1));
  HIPCHK(hipMemsetAsync(d_v2.p, 0xff, sizeof(unsigned long long), 0));
  hipLaunchKernelGGL(k_msk_labels, dim3(grid_for(nI, 256, 1 << 16)), block, 0, 0, nI, (const int32_t *)d_label.p, L,
                     d_v2.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(&viol, d_v2.p, sizeof(viol), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("check"));
  if (viol != ~0ull)
    return fail(TEHMM_ERR_ARG, who + ": interval " + std::to_string(viol) + " of the prediction has a label outside [0, L)");
  MskFill f;
  f.m = m.view;
  f.iv = iv.view;
  f.label = d_label.p;
  f.two = d_two.p;
  f.one = d_one.p;
  f.only_default = only_default ? 1 : 0;
  f.max_len = max_len;
  HIPCHK(d_out.alloc((size_t)nM));
  HIPCHK(hipMemsetAsync(d_v2.p, 0xff, sizeof(unsigned long long), 0));
  hipLaunchKernelGGL(k_msk_fill, dim3(grid_for(nM, 256, 1 << 16)), block, 0, 0, f, d_out.p, d_v2.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(&viol, d_v2.p, sizeof(viol), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("fill"));
  if (viol != ~0ull)
    return fail(TEHMM_ERR_ARG, who + ": mask " + std::to_string(viol) +
                                   " overlaps a flanking interval of the prediction without abutting it");
  HIPCHK(hipMemcpy(out_label, d_out.p, (size_t)nM * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_msk_timing));
  return TEHMM_OK;
}
