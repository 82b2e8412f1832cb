// tehmm_compare_host.inc -- host side of the kernels in tehmm_compare.hip.h (included by tehmm_hip.hip, behind
// tehmm_segment_host.inc whose SegClock it uses): the checks, the two comparisons and the run merge on interval lists.

namespace {

thread_local std::vector<std::pair<const char *, double>> t_cmp_timing;      // device passes of the last call

struct CmpDev {
  DBuf<int32_t> chrom, label;
  DBuf<int64_t> start, end;
  CmpList view;
  int upload(int64_t n, const int32_t *c, const int64_t *s, const int64_t *e, const int32_t *l) {
    HIPCHK(chrom.upload(c, (size_t)n));
    HIPCHK(start.upload(s, (size_t)n));
    HIPCHK(end.upload(e, (size_t)n));
    HIPCHK(label.upload(l, (size_t)n));
    view.n = n;
    view.chrom = chrom.p;
    view.start = start.p;
    view.end = end.p;
    view.label = label.p;
    return TEHMM_OK;
  }
};

// what every entry point checks before any device call
int cmp_list_args(const char *who, int64_t n, const int32_t *c, const int64_t *s, const int64_t *e, const int32_t *l) {
  if (!c || !s || !e || !l) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL list");
  if (n < 1) return fail(TEHMM_ERR_ARG, std::string(who) + ": a list holds at least one interval");
  if (n > 0x7fffffffll) return fail(TEHMM_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 intervals in a list");
  return TEHMM_OK;
}

int cmp_label_args(const char *who, int L) {
  if (L < 1) return fail(TEHMM_ERR_ARG, std::string(who) + ": L < 1");
  if (L > TEHMM_CMP_MAX_LABELS) return fail(TEHMM_ERR_UNSUPPORTED, std::string(who) + ": more than 2048 labels");
  return TEHMM_OK;
}

constexpr int kCmpGridCap = 2048;      // workgroups of the grid-stride kernels (each flushes one LDS matrix)

// validity of both lists, then equal cover: *which = 0, or the list (1, 2) and *where the index of the first offender
int cmp_check_dev(const CmpDev &a, const CmpDev &b, int L, int *which, int64_t *where, const char **what) {
  DBuf<unsigned long long> d_viol;
  HIPCHK(d_viol.alloc(2));
  unsigned long long v[2];
  const int grid = grid_for(a.view.n + b.view.n, 256, kCmpGridCap);
  *which = 0;
  *where = -1;
  for (int pass = 0; pass < 2; ++pass) {
    HIPCHK(hipMemsetAsync(d_viol.p, 0xff, sizeof(v), 0));
    if (pass == 0) hipLaunchKernelGGL(k_cmp_valid, dim3(grid), dim3(256), 0, 0, a.view, b.view, L, d_viol.p);
    else hipLaunchKernelGGL(k_cmp_cover, dim3(grid), dim3(256), 0, 0, a.view, b.view, d_viol.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(v, d_viol.p, sizeof(v), hipMemcpyDeviceToHost));
    for (int w = 0; w < 2; ++w)
      if (v[w] != ~0ull) {
        *which = w + 1;
        *where = (int64_t)v[w];
        *what = pass == 0 ? "is empty, out of order, overlaps its predecessor or has a label outside [0, L)"
                          : "has a region boundary that the other list lacks: the lists do not cover the same bases";
        return TEHMM_OK;
      }
  }
  return TEHMM_OK;
}

// upload + check of a comparison: TEHMM_ERR_ARG with the offender's name when the lists cannot be compared
int cmp_prepare(const char *who, CmpDev &a, CmpDev &b, int L, int64_t n1, const int32_t *c1, const int64_t *s1,
                const int64_t *e1, const int32_t *l1, int64_t n2, const int32_t *c2, const int64_t *s2,
                const int64_t *e2, const int32_t *l2, SegClock &clk) {
  int rc = a.upload(n1, c1, s1, e1, l1);
  if (rc == TEHMM_OK) rc = b.upload(n2, c2, s2, e2, l2);
  if (rc) return rc;
  HIPCHK(clk.mark("upload"));
  int which = 0;
  int64_t where = -1;
  const char *what = "";
  rc = cmp_check_dev(a, b, L, &which, &where, &what);
  if (rc) return rc;
  HIPCHK(clk.mark("check"));
  if (which)
    return fail(TEHMM_ERR_ARG, std::string(who) + ": interval " + std::to_string((long long)where) + " of list " +
                                   std::to_string(which) + " " + what);
  return TEHMM_OK;
}

}  // namespace

int tehmm_compare_lds_labels(void) { return TEHMM_CMP_LDS_LABELS; }

int64_t tehmm_compare_block_items(void) { return TEHMM_SCAN_BLOCK; }

int tehmm_compare_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_compare_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_cmp_timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_intervals_check(int64_t n1, const int32_t *chrom1, const int64_t *start1, const int64_t *end1,
                          const int32_t *label1, int64_t n2, const int32_t *chrom2, const int64_t *start2,
                          const int64_t *end2, const int32_t *label2, int L, int *which, int64_t *where) {
  const char *who = "tehmm_intervals_check";
  t_cmp_timing.clear();
  if (!which || !where) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL output");
  int rc = cmp_label_args(who, L);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n1, chrom1, start1, end1, label1);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n2, chrom2, start2, end2, label2);
  if (rc) return rc;
  SegClock clk;
  CmpDev a, b;
  HIPCHK(clk.mark("start"));
  rc = a.upload(n1, chrom1, start1, end1, label1);
  if (rc == TEHMM_OK) rc = b.upload(n2, chrom2, start2, end2, label2);
  if (rc) return rc;
  HIPCHK(clk.mark("upload"));
  const char *what = "";
  rc = cmp_check_dev(a, b, L, which, where, &what);
  if (rc) return rc;
  if (*which)
    g_err = std::string(who) + ": interval " + std::to_string((long long)*where) + " of list " +
            std::to_string(*which) + " " + what;
  HIPCHK(clk.mark("check"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_cmp_timing));
  return TEHMM_OK;
}

int tehmm_compare_base(int64_t n1, const int32_t *chrom1, const int64_t *start1, const int64_t *end1,
                       const int32_t *label1, int64_t n2, const int32_t *chrom2, const int64_t *start2,
                       const int64_t *end2, const int32_t *label2, int L, int64_t *conf, int64_t *first) {
  const char *who = "tehmm_compare_base";
  t_cmp_timing.clear();
  if (!conf) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL output");
  int rc = cmp_label_args(who, L);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n1, chrom1, start1, end1, label1);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n2, chrom2, start2, end2, label2);
  if (rc) return rc;
  SegClock clk;
  CmpDev a, b;
  HIPCHK(clk.mark("start"));
  rc = cmp_prepare(who, a, b, L, n1, chrom1, start1, end1, label1, n2, chrom2, start2, end2, label2, clk);
  if (rc) return rc;
  const size_t cells = (size_t)L * (size_t)L;
  DBuf<unsigned long long> d_conf, d_first;
  HIPCHK(d_conf.alloc(cells));
  HIPCHK(hipMemsetAsync(d_conf.p, 0, cells * sizeof(unsigned long long), 0));
  if (first) {
    HIPCHK(d_first.alloc(cells));
    HIPCHK(hipMemsetAsync(d_first.p, 0xff, cells * sizeof(unsigned long long), 0));
  }
  const dim3 grid(grid_for(n1 + n2, 256, kCmpGridCap)), block(256);
  if (L <= TEHMM_CMP_LDS_LABELS)
    hipLaunchKernelGGL((k_cmp_base<true>), grid, block, cells * sizeof(unsigned long long), 0, a.view, b.view, L,
                       d_conf.p, d_first.p);
  else hipLaunchKernelGGL((k_cmp_base<false>), grid, block, 0, 0, a.view, b.view, L, d_conf.p, d_first.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("base"));
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "matrix cell");
  HIPCHK(hipMemcpy(conf, d_conf.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (first) HIPCHK(hipMemcpy(first, d_first.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_cmp_timing));
  return TEHMM_OK;
}

int tehmm_compare_intervals(int64_t n_true, const int32_t *chrom_t, const int64_t *start_t, const int64_t *end_t,
                            const int32_t *label_t, int64_t n_pred, const int32_t *chrom_p, const int64_t *start_p,
                            const int64_t *end_p, const int32_t *label_p, int L, double threshold, int use_pred_len,
                            int allow_multiple, int64_t *n_hit, int64_t *len_hit, int64_t *n_miss, int64_t *len_miss,
                            int64_t *conf, int64_t *first) {
  const char *who = "tehmm_compare_intervals";
  t_cmp_timing.clear();
  if (!n_hit || !len_hit || !n_miss || !len_miss || !conf) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL output");
  if (threshold != threshold) return fail(TEHMM_ERR_ARG, std::string(who) + ": threshold is NaN");
  int rc = cmp_label_args(who, L);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n_true, chrom_t, start_t, end_t, label_t);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n_pred, chrom_p, start_p, end_p, label_p);
  if (rc) return rc;
  SegClock clk;
  CmpDev t, p;
  HIPCHK(clk.mark("start"));
  rc = cmp_prepare(who, t, p, L, n_true, chrom_t, start_t, end_t, label_t, n_pred, chrom_p, start_p, end_p, label_p,
                   clk);
  if (rc) return rc;
  CmpIntervalOpt o;
  o.L = L;
  o.threshold = threshold;
  o.use_pred_len = use_pred_len ? 1 : 0;
  o.allow_multiple = allow_multiple ? 1 : 0;
  const size_t cells = (size_t)cmp_interval_cells(L);
  const bool lds = L <= TEHMM_CMP_LDS_LABELS;
  const size_t shmem = lds ? cells * sizeof(unsigned long long) : 0;
  DBuf<unsigned long long> d_out, d_nlong, d_first;
  DBuf<int32_t> d_long;
  HIPCHK(d_out.alloc(cells));
  HIPCHK(d_nlong.alloc(1));
  HIPCHK(d_long.alloc((size_t)n_true));
  HIPCHK(hipMemsetAsync(d_out.p, 0, cells * sizeof(unsigned long long), 0));
  HIPCHK(hipMemsetAsync(d_nlong.p, 0, sizeof(unsigned long long), 0));
  const size_t LL = (size_t)L * (size_t)L, l = (size_t)L;
  if (first) {
    HIPCHK(d_first.alloc(LL));
    HIPCHK(hipMemsetAsync(d_first.p, 0xff, LL * sizeof(unsigned long long), 0));
  }
  const dim3 grid(grid_for(n_true, 256, kCmpGridCap)), block(256);
  if (lds)
    hipLaunchKernelGGL((k_cmp_intervals<true>), grid, block, shmem, 0, t.view, p.view, o, d_out.p, d_first.p, d_long.p,
                       d_nlong.p);
  else
    hipLaunchKernelGGL((k_cmp_intervals<false>), grid, block, 0, 0, t.view, p.view, o, d_out.p, d_first.p, d_long.p,
                       d_nlong.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("intervals"));
  unsigned long long n_long = 0;
  HIPCHK(hipMemcpy(&n_long, d_nlong.p, sizeof(n_long), hipMemcpyDeviceToHost));
  if (n_long > (unsigned long long)n_true) return fail(TEHMM_ERR_HIP, std::string(who) + ": inconsistent long-range count");
  if (n_long > 0) {      // the kernel boundary orders the two passes
    const dim3 lgrid(grid_for((int64_t)n_long, 4, kCmpGridCap));
    if (lds)
      hipLaunchKernelGGL((k_cmp_intervals_long<true>), lgrid, block, shmem, 0, t.view, p.view, o, d_out.p,
                         d_first.p, (const int32_t *)d_long.p, (int64_t)n_long);
    else
      hipLaunchKernelGGL((k_cmp_intervals_long<false>), lgrid, block, 0, 0, t.view, p.view, o, d_out.p,
                         d_first.p, (const int32_t *)d_long.p, (int64_t)n_long);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("long_ranges"));
  }
  std::vector<int64_t> out(cells);
  HIPCHK(hipMemcpy(out.data(), d_out.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (first) HIPCHK(hipMemcpy(first, d_first.p, LL * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::memcpy(conf, out.data(), LL * sizeof(int64_t));
  std::memcpy(n_hit, out.data() + LL, l * sizeof(int64_t));
  std::memcpy(len_hit, out.data() + LL + l, l * sizeof(int64_t));
  std::memcpy(n_miss, out.data() + LL + 2 * l, l * sizeof(int64_t));
  std::memcpy(len_miss, out.data() + LL + 3 * l, l * sizeof(int64_t));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_cmp_timing));
  return TEHMM_OK;
}

int tehmm_merge_runs(int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, const int32_t *label,
                     int L, const int32_t *lut, int64_t cap, int32_t *out_chrom, int64_t *out_start, int64_t *out_end,
                     int32_t *out_label, int64_t *n_out) {
  const char *who = "tehmm_merge_runs";
  t_cmp_timing.clear();
  if (!n_out || cap < 0 || (cap > 0 && (!out_chrom || !out_start || !out_end || !out_label)))
    return fail(TEHMM_ERR_ARG, std::string(who) + ": bad argument");
  int rc = cmp_label_args(who, L);
  if (rc == TEHMM_OK) rc = cmp_list_args(who, n, chrom, start, end, label);
  if (rc) return rc;
  SegClock clk;
  CmpDev a;
  DBuf<int32_t> d_lut, d_mapped, d_oc, d_ol;
  DBuf<int64_t> d_os, d_oe, d_tot;
  DBuf<uint8_t> d_head;
  DBuf<unsigned> d_blk;
  DBuf<unsigned long long> d_viol;
  HIPCHK(clk.mark("start"));
  rc = a.upload(n, chrom, start, end, label);
  if (rc) return rc;
  if (lut) HIPCHK(d_lut.upload(lut, (size_t)L));
  HIPCHK(clk.mark("upload"));
  const int64_t nb = (n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  HIPCHK(d_mapped.alloc((size_t)n));
  HIPCHK(d_head.alloc((size_t)n));
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_tot.alloc(1));
  HIPCHK(d_viol.alloc(1));
  HIPCHK(hipMemsetAsync(d_viol.p, 0xff, sizeof(unsigned long long), 0));
  const dim3 block(256);
  hipLaunchKernelGGL(k_mrg_flags, dim3(grid_for(n, 256, 1 << 16)), block, 0, 0, a.view, L, (const int32_t *)d_lut.p,
                     d_mapped.p, d_head.p, d_viol.p);
  hipLaunchKernelGGL(k_seg_count, dim3((unsigned)nb), block, 0, 0, n, (const uint8_t *)d_head.p, d_blk.p);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), block, 0, 0, nb, d_blk.p, d_tot.p);
  HIPCHK(hipGetLastError());
  int64_t nt = 0;
  unsigned long long viol = 0;
  HIPCHK(hipMemcpy(&nt, d_tot.p, sizeof(nt), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&viol, d_viol.p, sizeof(viol), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("heads"));
  if (viol != ~0ull)
    return fail(TEHMM_ERR_ARG, std::string(who) + ": interval " + std::to_string(viol) + " has a label outside [0, L)");
  if (nt < 1 || nt > n) return fail(TEHMM_ERR_HIP, std::string(who) + ": inconsistent run count");
  *n_out = nt;
  if (nt <= cap) {
    HIPCHK(d_oc.alloc((size_t)nt));
    HIPCHK(d_os.alloc((size_t)nt));
    HIPCHK(d_oe.alloc((size_t)nt));
    HIPCHK(d_ol.alloc((size_t)nt));
    hipLaunchKernelGGL(k_mrg_scatter, dim3((unsigned)nb), block, 0, 0, a.view, (const int32_t *)d_mapped.p,
                       (const uint8_t *)d_head.p, (const unsigned *)d_blk.p, d_oc.p, d_os.p, d_oe.p, d_ol.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("scatter"));
    HIPCHK(hipMemcpy(out_chrom, d_oc.p, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_start, d_os.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_end, d_oe.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_label, d_ol.p, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(clk.mark("download"));
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_cmp_timing));
  return TEHMM_OK;
}
