// tehmm_cyk_host.inc -- host side of the kernels in tehmm_cyk.hip.h (included by tehmm_hip.hip, behind
// tehmm_segment_host.inc whose SegClock it uses): CYK decode of a batch of intervals under the grammar model
// (DESIGN.md section 5t).

namespace {

thread_local std::vector<std::pair<const char *, double>> t_cyk_timing;

// A diagonal takes the workgroup-per-cell form when a cell has at least this many splits per lane of a workgroup and
// the wave-per-cell form would leave the device short of waves (DESIGN.md 5t: occupancy arithmetic, not measured).
constexpr int kCykWgMinSize = 257;          // size - 1 >= 256 splits: every lane of the workgroup has one
constexpr int64_t kCykWgMaxGroups = 4096;   // 256 CUs x 4 SIMDs x 4 waves

// Bytes of device memory a call needs: THE workspace formula (DESIGN.md 5t).
//   dp     8 M L^2 per interval   one square per state, both copies of the upper triangle in it
//   em     8 M total              stack 12 (total + n)     trace 8 total     alignment 2 total
//   lists  17 M^3 + 9 M^2 at most, items and results 56 n, status 16 n
int64_t cyk_workspace_bytes(int n, const int64_t *lens, int M) {
  int64_t total = 0, cells = 0;
  for (int t = 0; t < n; ++t) {
    total += lens[t];
    cells += lens[t] * lens[t];
  }
  const int64_t m = M;
  return 8 * m * cells + (8 * m + 12 + 8 + 2) * total + 17 * m * m * m + 9 * m * m + 64 * m + 84 * (int64_t)n + 4096;
}

// the largest single interval whose workspace fits the budget (0: none)
int64_t cyk_max_len(int M, int64_t budget) {
  int64_t lo = 0, hi = (int64_t)1 << 24;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (cyk_workspace_bytes(1, &mid, M) <= budget) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

int cyk_budget(int64_t *budget) {
  if (const char *e = std::getenv("TEHMM_CYK_MAX_BYTES")) {      // tests and tight hosts
    *budget = std::atoll(e);
    return TEHMM_OK;
  }
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  *budget = (int64_t)(total_b / 10 * 8);                         // (blocks cached by the device pool are not "free")
  return TEHMM_OK;
}

struct CykCall {
  const char *who;
  int n;
  const int64_t *offsets;
  int M;
  const double *em;
  const uint16_t *al;
  int defSym;
  const uint8_t *is_nest;
  const double *lp1, *lp2, *priors, *start;
};

// everything up to and including the fill; dp and items stay on the device for what follows
struct CykRun {
  DBuf<double> d_dp, d_em, d_h1lp, d_h2lp, d_priors, d_start;
  DBuf<uint16_t> d_al;
  DBuf<uint8_t> d_nest, d_h1r1, d_h1r2, d_h2r;
  DBuf<int32_t> d_h1off, d_h2off;
  DBuf<CykItem> d_items;
  std::vector<CykItem> items;
  CykModel mod;
  SegClock clk;
};

int cyk_fill(const CykCall &c, CykRun &r) {
  const std::string who = c.who;
  if (c.n < 0 || c.M < 1 || !c.offsets || !c.is_nest || !c.lp1 || !c.lp2 || !c.priors || !c.start)
    return fail(TEHMM_ERR_ARG, who + ": bad argument");
  if (c.M > TEHMM_CYK_MAX_STATES) return fail(TEHMM_ERR_UNSUPPORTED, who + ": M > 64");
  const int n = c.n, M = c.M;
  if (c.offsets[0] != 0) return fail(TEHMM_ERR_ARG, who + ": offsets must start at 0");
  std::vector<int64_t> lens((size_t)n);
  for (int t = 0; t < n; ++t) {
    lens[(size_t)t] = c.offsets[t + 1] - c.offsets[t];
    if (lens[(size_t)t] < 1) return fail(TEHMM_ERR_ARG, who + ": every interval needs at least one row");
  }
  const int64_t total = c.offsets[n];
  if (!c.em) return fail(TEHMM_ERR_ARG, who + ": emLogProbs is NULL");
  // ---- does it fit: before anything is allocated ------------------------------------------------------------------
  int64_t budget = 0;
  int rc = cyk_budget(&budget);
  if (rc != TEHMM_OK) return rc;
  const int64_t lmax_fit = cyk_max_len(M, budget);
  const int64_t lmax = *std::max_element(lens.begin(), lens.end());
  if (lmax > lmax_fit || cyk_workspace_bytes(n, lens.data(), M) > budget)
    return fail(TEHMM_ERR_UNSUPPORTED, who + ": the workspace of these intervals (" +
                                           std::to_string(cyk_workspace_bytes(n, lens.data(), M)) + " bytes, longest interval " +
                                           std::to_string(lmax) + ") does not fit; the largest single interval that fits at M = " +
                                           std::to_string(M) + " is L = " + std::to_string(lmax_fit) +
                                           " (cut the intervals, teHmmEval --slice)");
  // ---- helper lists (cfg.py:121-158): every production above -inf, -1e100 included ---------------------------------
  std::vector<int32_t> h1off(1, 0), h2off(1, 0);
  std::vector<uint8_t> h1r1, h1r2, h2r;
  std::vector<double> h1lp, h2lp;
  for (int x = 0; x < M; ++x) {
    for (int r1 = 0; r1 < M; ++r1)
      for (int r2 = 0; r2 < M; ++r2) {
        const double v = c.lp1[((size_t)x * M + r1) * M + r2];
        if (v > -INFINITY) {
          h1r1.push_back((uint8_t)r1);
          h1r2.push_back((uint8_t)r2);
          h1lp.push_back(v);
        }
      }
    h1off.push_back((int32_t)h1lp.size());
    for (int rr = 0; rr < M; ++rr) {
      const double v = c.lp2[(size_t)x * M + rr];
      if (v > -INFINITY) {
        h2r.push_back((uint8_t)rr);
        h2lp.push_back(v);
      }
    }
    h2off.push_back((int32_t)h2lp.size());
  }
  // ---- items, longest first: the intervals a diagonal still concerns are a prefix -----------------------------------
  r.items.resize((size_t)n);
  int64_t dp_elems = 0;
  for (int t = 0; t < n; ++t) {
    CykItem &it = r.items[(size_t)t];
    it.row0 = c.offsets[t];
    it.dp0 = dp_elems;
    it.L = (int32_t)lens[(size_t)t];
    it.idx = t;
    dp_elems += (int64_t)M * lens[(size_t)t] * lens[(size_t)t];
  }
  std::stable_sort(r.items.begin(), r.items.end(), [](const CykItem &a, const CykItem &b) { return a.L > b.L; });
  HIPCHK(r.clk.mark("start"));
  HIPCHK(r.d_em.upload(c.em, (size_t)total * M));
  if (c.al) HIPCHK(r.d_al.upload(c.al, (size_t)total));
  HIPCHK(r.d_nest.upload(c.is_nest, (size_t)M));
  HIPCHK(r.d_h1off.upload(h1off.data(), h1off.size()));
  HIPCHK(r.d_h1r1.upload(h1r1.data(), h1r1.size()));
  HIPCHK(r.d_h1r2.upload(h1r2.data(), h1r2.size()));
  HIPCHK(r.d_h1lp.upload(h1lp.data(), h1lp.size()));
  HIPCHK(r.d_h2off.upload(h2off.data(), h2off.size()));
  HIPCHK(r.d_h2r.upload(h2r.data(), h2r.size()));
  HIPCHK(r.d_h2lp.upload(h2lp.data(), h2lp.size()));
  HIPCHK(r.d_priors.upload(c.priors, (size_t)M * 2));
  HIPCHK(r.d_start.upload(c.start, (size_t)M));
  HIPCHK(r.d_items.upload(r.items.data(), r.items.size()));
  HIPCHK(r.d_dp.alloc((size_t)dp_elems));
  CykModel &mod = r.mod;
  mod.M = M;
  mod.defSym = c.defSym;
  mod.is_nest = r.d_nest.p;
  mod.h1_off = r.d_h1off.p;
  mod.h1_r1 = r.d_h1r1.p;
  mod.h1_r2 = r.d_h1r2.p;
  mod.h1_lp = r.d_h1lp.p;
  mod.h2_off = r.d_h2off.p;
  mod.h2_r = r.d_h2r.p;
  mod.h2_lp = r.d_h2lp.p;
  mod.logPriors = r.d_priors.p;
  mod.log_start = r.d_start.p;
  mod.em = r.d_em.p;
  mod.al = c.al ? r.d_al.p : nullptr;
  if (n == 0) return TEHMM_OK;
  HIPCHK(r.clk.mark("upload"));
  constexpr int kGridY = 65535;
  for (int y0 = 0; y0 < n; y0 += kGridY) {
    const int ny = std::min(kGridY, n - y0);
    const int64_t e = (int64_t)M * r.items[(size_t)y0].L * r.items[(size_t)y0].L;
    hipLaunchKernelGGL(k_cyk_init, dim3((unsigned)grid_for(e, 256, 1 << 16), (unsigned)ny), dim3(256), 0, 0, mod,
                       (const CykItem *)(r.d_items.p + y0), r.d_dp.p);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(r.clk.mark("init"));
  static const int wg_min = [] {
    const char *e = std::getenv("TEHMM_CYK_WG_MIN_SIZE");      // measurement knob: the first size of the workgroup form
    return e ? std::max(2, std::atoi(e)) : kCykWgMinSize;
  }();
  int active = n;                                 // items with L >= size
  for (int size = 2; size <= (int)lmax; ++size) {
    while (active > 0 && r.items[(size_t)active - 1].L < size) --active;
    const int splits = size - 1;
    int tpc = splits <= 8 ? 8 : splits <= 16 ? 16 : splits <= 32 ? 32 : 64;
    if (size >= wg_min) {
      int64_t groups = 0;                         // (cell, state) groups of this diagonal, counted up to the bound
      for (int t = 0; t < active && groups < kCykWgMaxGroups; ++t) groups += (int64_t)(r.items[(size_t)t].L - size + 1) * M;
      if (groups < kCykWgMaxGroups) tpc = 256;
    }
    const int gpb = 256 / tpc;
    for (int y0 = 0; y0 < active; y0 += kGridY) {
      const int ny = std::min(kGridY, active - y0);
      const int64_t groups = (int64_t)(r.items[(size_t)y0].L - size + 1) * M;
      const dim3 grid((unsigned)((groups + gpb - 1) / gpb), (unsigned)ny), block(256);
      switch (tpc) {
        case 8: hipLaunchKernelGGL(k_cyk_fill<8>, grid, block, 0, 0, mod, (const CykItem *)r.d_items.p, y0, size, r.d_dp.p); break;
        case 16: hipLaunchKernelGGL(k_cyk_fill<16>, grid, block, 0, 0, mod, (const CykItem *)r.d_items.p, y0, size, r.d_dp.p); break;
        case 32: hipLaunchKernelGGL(k_cyk_fill<32>, grid, block, 0, 0, mod, (const CykItem *)r.d_items.p, y0, size, r.d_dp.p); break;
        case 64: hipLaunchKernelGGL(k_cyk_fill<64>, grid, block, 0, 0, mod, (const CykItem *)r.d_items.p, y0, size, r.d_dp.p); break;
        default: hipLaunchKernelGGL(k_cyk_fill<256>, grid, block, 0, 0, mod, (const CykItem *)r.d_items.p, y0, size, r.d_dp.p); break;
      }
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(r.clk.mark("fill"));
  return TEHMM_OK;
}

void cyk_finish_timing(CykRun &r, std::chrono::steady_clock::time_point wall0) {
  std::vector<std::pair<const char *, double>> marks;
  // (the last mark was recorded behind a blocking copy: it still has to complete before it can be read)
  if (hipDeviceSynchronize() == hipSuccess && r.clk.finish(marks) == hipSuccess) t_cyk_timing = marks;
  t_cyk_timing.emplace_back("wall", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count());
}

}  // namespace

int tehmm_cyk_decode(int n_intervals, const int64_t *offsets, int M, const double *emLogProbs, const uint16_t *alignment,
                     int defAlignmentSymbol, const uint8_t *is_nest, const double *logProbs1, const double *logProbs2,
                     const double *logPriors, const double *log_start, double *scores, int64_t *top, double *trace) {
  const std::string who = "tehmm_cyk_decode";
  t_cyk_timing.clear();
  const auto wall0 = std::chrono::steady_clock::now();
  if (n_intervals > 0 && (!scores || !top || !trace)) return fail(TEHMM_ERR_ARG, who + ": NULL result array");
  CykCall c = {"tehmm_cyk_decode", n_intervals, offsets, M, emLogProbs, alignment, defAlignmentSymbol, is_nest,
               logProbs1, logProbs2, logPriors, log_start};
  CykRun r;
  int rc = cyk_fill(c, r);
  if (rc != TEHMM_OK || n_intervals == 0) return rc;
  const int n = n_intervals;
  const int64_t total = offsets[n];
  DBuf<double> d_scores, d_trace;
  DBuf<int64_t> d_top;
  DBuf<int32_t> d_stack, d_status;
  HIPCHK(d_scores.alloc((size_t)n));
  HIPCHK(d_top.alloc((size_t)n));
  HIPCHK(d_trace.alloc((size_t)total));
  HIPCHK(d_stack.alloc((size_t)(3 * (total + n))));
  HIPCHK(d_status.alloc((size_t)n * 4));
  HIPCHK(hipMemsetAsync(d_status.p, 0, (size_t)n * 4 * sizeof(int32_t), 0));
  hipLaunchKernelGGL(k_cyk_score, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, r.mod, (const CykItem *)r.d_items.p, n,
                     (const double *)r.d_dp.p, d_scores.p, d_top.p);
  hipLaunchKernelGGL(k_cyk_trace, dim3((unsigned)n), dim3(256), 0, 0, r.mod, (const CykItem *)r.d_items.p,
                     (const double *)r.d_dp.p, (const int64_t *)d_top.p, d_stack.p, d_trace.p, d_status.p);
  HIPCHK(hipGetLastError());
  HIPCHK(r.clk.mark("traceback"));
  std::vector<int32_t> status((size_t)n * 4);
  HIPCHK(hipMemcpy(status.data(), d_status.p, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(scores, d_scores.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(top, d_top.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(trace, d_trace.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(r.clk.mark("copy_back"));
  cyk_finish_timing(r, wall0);
  for (int t = 0; t < n; ++t)
    if (status[(size_t)t * 4] != 0)
      return fail(TEHMM_ERR_ARG, who + ": interval " + std::to_string(t) + " has no derivation: cell (" +
                                     std::to_string(status[(size_t)t * 4 + 1]) + ", " + std::to_string(status[(size_t)t * 4 + 2]) +
                                     ") of state " + std::to_string(status[(size_t)t * 4 + 3]) +
                                     (status[(size_t)t * 4] == 1 ? " is -inf" : " matches no production (internal error)"));
  return TEHMM_OK;
}

int tehmm_cyk_get_dp(int64_t L, int M, const double *emLogProbs, const uint16_t *alignment, int defAlignmentSymbol,
                     const uint8_t *is_nest, const double *logProbs1, const double *logProbs2, const double *logPriors,
                     const double *log_start, double *dp) {
  const std::string who = "tehmm_cyk_get_dp";
  t_cyk_timing.clear();
  const auto wall0 = std::chrono::steady_clock::now();
  if (!dp || L < 1) return fail(TEHMM_ERR_ARG, who + ": bad argument");
  const int64_t offsets[2] = {0, L};
  CykCall c = {"tehmm_cyk_get_dp", 1, offsets, M, emLogProbs, alignment, defAlignmentSymbol, is_nest,
               logProbs1, logProbs2, logPriors, log_start};
  CykRun r;
  int rc = cyk_fill(c, r);
  if (rc != TEHMM_OK) return rc;
  std::vector<double> sq((size_t)(M * L * L));
  HIPCHK(hipMemcpy(sq.data(), r.d_dp.p, sq.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(r.clk.mark("copy_back"));
  for (int64_t i = 0; i < L; ++i)
    for (int64_t j = 0; j < L; ++j)
      for (int x = 0; x < M; ++x)
        dp[(i * L + j) * M + x] = j >= i ? sq[(size_t)((x * L + i) * L + j)] : -INFINITY;
  // (the second copy has to agree: the accessor is a test's view of both)
  for (int x = 0; x < M; ++x)
    for (int64_t i = 0; i < L; ++i)
      for (int64_t j = i + 1; j < L; ++j) {
        const double a = sq[(size_t)((x * L + i) * L + j)], b = sq[(size_t)((x * L + j) * L + i)];
        if (std::memcmp(&a, &b, sizeof(double)) != 0) return fail(TEHMM_ERR_HIP, who + ": the two copies of a cell differ");
      }
  cyk_finish_timing(r, wall0);
  return TEHMM_OK;
}

int tehmm_cyk_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_cyk_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_cyk_timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

// the workspace formula, for callers that plan their slices (no device call)
int64_t tehmm_cyk_workspace_bytes(int n_intervals, const int64_t *lengths, int M) {
  if (n_intervals < 0 || (n_intervals > 0 && !lengths) || M < 1) return fail(TEHMM_ERR_ARG, "tehmm_cyk_workspace_bytes: bad argument");
  return cyk_workspace_bytes(n_intervals, lengths, M);
}
