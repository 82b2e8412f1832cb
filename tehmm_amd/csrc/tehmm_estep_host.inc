// tehmm_estep_host.inc -- host side of the Baum-Welch E-step for N <= 128 (included by tehmm_hip.hip): three routes to
// one statistics buffer (layout: tehmm_aux.hip.h) and the driver that picks one, estep_accumulate:
//   estep_fused       the fused posterior passes + the reductions of tehmm_estep.hip.h (N < 64, no segment ratios)
//   estep_wide        the item-parallel passes of tehmm_wide.hip.h + tehmm_wide_estep.hip.h (64 <= N <= 128, or ratios)
//   estep_sequential  k_fb_coop + k_estep_accum over groups of intervals that fit a fixed workspace (N < 64)

// Slots of b->ev[] / b->evX[] the routes record.  The passes (launch_fused_fb; wide_post_attempt, wide_verdict) record
// kEvFwdEnd and kEvBwdEnd in both routes; the slots around them differ, hence two names for 7 and 9.
enum EstepEvent {
  kEvStart = 10,           // both: first device work of the call
  kEvFwdEnd = 8,           // both: end of the forward pass
  kEvBwdEnd = 6,           // fused: end of the backward pass; wide: the links have verified
  kEvFusedChainEnd = 7,    // fused: end of the exact backward chain
  kEvFusedReduceEnd = 9,
  kEvWideEmisEnd = 12,     // wide: end of the emission rows
  kEvWideAttempt = 9,      // wide: start of the (last) attempt of the passes
  kEvWideReduceEnd = 7,
  kEvLdsDone = 11,         // both: the LDS histograms are folded (their own stream)
};
enum EstepForkEvent {      // b->evX[]
  kEvxFork = 0,            // the reductions' streams start behind this
  kEvxRowsDone = 1,        // the one-hot row product is folded (its own stream)
};

// What a route returns: it ran, it declined (the driver tries the next route), or an error.
struct EstepOutcome {
  enum Kind { Ran, Declined, Error } kind;
  int rc;                                               // the TEHMM_ERR_* code of an Error, else TEHMM_OK
  EstepOutcome(Kind k) : kind(k), rc(TEHMM_OK) {}
  EstepOutcome(int err) : kind(Error), rc(err) {}       // (implicit: what HIPCHK and fail() return)
};

// ---- pieces the routes share ---------------------------------------------------------------------------------------
// Per-interval scalars on the device.  (ensure_workspace allocates the same three under another condition -- whenever
// the posterior rows are missing -- so it keeps its own lines.)
static int ensure_interval_scalars(tehmm_batch *b) {
  if (!b->fwd_lp.p || !b->dead.p) {
    HIPCHK(b->fwd_lp.alloc((size_t)b->n + 1));
    HIPCHK(b->dead.alloc((size_t)b->n + 1));
    if (!b->first_good.p) HIPCHK(b->first_good.alloc((size_t)b->n + 1));
  }
  return TEHMM_OK;
}

// Results of the intervals `ids` (nullptr: all of them, in their own order), once the stream is through: log-likelihoods
// added to *lp_out and kept per interval in b->h_fwd_lp (NaN where dead), dead flags or-ed into *dead_out.  d_dead ==
// nullptr: the route accepts no dead interval.  Empty intervals are left out: no kernel writes their slots.
static int estep_results(tehmm_batch *b, const double *d_lp, const int *d_dead, const std::vector<int> *ids, double *lp_out,
                         int *dead_out) {
  std::vector<double> lp((size_t)b->n);
  std::vector<int> dead((size_t)b->n, 0);
  HIPCHK(hipMemcpy(lp.data(), d_lp, (size_t)b->n * sizeof(double), hipMemcpyDeviceToHost));
  if (d_dead) HIPCHK(hipMemcpy(dead.data(), d_dead, (size_t)b->n * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < (ids ? ids->size() : (size_t)b->n); ++i) {
    const int id = ids ? (*ids)[i] : (int)i;
    if (b->h_len[(size_t)id] <= 0) continue;
    *lp_out += lp[(size_t)id];
    *dead_out |= dead[(size_t)id];
    b->h_fwd_lp[(size_t)id] = dead[(size_t)id] ? std::nan("") : lp[(size_t)id];
  }
  return TEHMM_OK;
}

// LDS histograms in 64-bit fixed point: positions one workgroup can add into one cell (its share of the units, in
// rounds of 8, x 16 items x positions per item and unit), and the binary point that keeps the largest sum `vmax` a
// workgroup can reach below 2^63
static int64_t hist_positions_per_wg(int64_t n_units, int gx, int64_t positions) {
  return ((n_units + (int64_t)gx * 8 - 1) / ((int64_t)gx * 8)) * 8 * 16 * positions;
}
static int hist_fixed_point_shift(double vmax) {
  int shift = 62;
  while (shift > 20 && vmax * std::ldexp(1.0, shift) >= 9.2e18) --shift;
  return shift;
}

// Rows of track k in a row table of the one-hot products, from `row` on: row -> observation column | symbol << 8 and
// row -> row of the global statistics table.  Returns the next free row.
static int fill_track_rows(const tehmm_model *m, int k, int row, int *info, int *grow) {
  for (int sy = 0; sy < m->rowcnt[k]; ++sy, ++row) {
    info[row] = (k & 255) | (sy << 8);
    grow[row] = m->rowbase[k] + sy;
  }
  return row;
}

// ---- sequential E-step: k_fb_coop + k_estep_accum ------------------------------------------------------------------
constexpr int kEstepChunk = 512;

template <int NT>
static void launch_estep(const tehmm_model *m, const IntervalTab &iv, const EmisTab &em, bool ratio, int n_iv, int n_chunks,
                         EstepWork &w, const double *tratios, hipStream_t st) {
  constexpr int CPB = NT <= 44 ? 64 : 32;
  const EmisTab emf = n_iv > 256 ? without_lds_tables(em) : em;
  size_t lds = ((size_t)4 * CPB * (NT + 1) + 4 * CPB + 5 * NT + (size_t)emf.lds_rows * NT) * sizeof(double);
  // k_estep_accum: a histogram per wave; w.seq_blocks workgroups share the chunks, every wave with a slot of w.part_seq
  size_t lds2 = (size_t)4 * std::max(1, m->lds_rows) * NT * sizeof(double) + (size_t)3 * m->K * sizeof(int) + 16;
  const int64_t ssz = stats_size(NT, m->R);
  const int gb = std::max(1, std::min(w.seq_blocks, (n_chunks + 3) / 4));
  (void)hipMemsetAsync(w.part_seq.p, 0, (size_t)gb * 4 * ssz * sizeof(double), st);
  bool_dispatch(ratio, [&](auto r) {
    allow_lds(k_fb_coop<NT, CPB, r>, lds);
    hipLaunchKernelGGL((k_fb_coop<NT, CPB, r>), dim3(n_iv), dim3(256), lds, st, iv, emf, m->N, m->A.p, m->lt.p, m->pi.p,
                       (const double *)(r ? tratios : nullptr), w.alpha.p, w.beta.p, w.fwd_lp.p, w.dead.p, w.wrows.p,
                       w.escale.p);
    allow_lds(k_estep_accum<NT, r>, lds2);
    hipLaunchKernelGGL((k_estep_accum<NT, r>), dim3(gb), dim3(256), lds2, st, iv, em, m->N, kEstepChunk,
                       w.chunk_iv.p, w.chunk_t0.p, n_chunks, w.alpha.p, w.beta.p, w.wrows.p, w.escale.p, w.part_seq.p, ssz);
  });
  hipLaunchKernelGGL(k_estep_accum_fold, dim3((unsigned)((ssz + 255) / 256)), dim3(256), 0, st, (const double *)w.part_seq.p,
                     gb * 4, ssz, w.stats_base);
}

static int estep_sequential(tehmm_model_t *m, tehmm_batch_t *b, bool ratio, double *dev_stats, double *lp_out,
                            int *dead_out) {
  const int N = m->N, NP = m->NP;
  // Intervals are processed in groups whose alpha / beta / w rows fit a fixed workspace
  // (3 x 8N + 4 bytes per position, 40 % of the free HBM): the 3 Gb training sets of config 4
  // never materialise whole-genome lattices.
  size_t free_b = 0, total_b = 0;
  (void)dev_mem_info(&free_b, &total_b);
  int64_t budget_bytes = (int64_t)((double)(free_b + (size_t)b->ew.rows_cap * (24 * N + 4)) * 0.4);
  if (budget_bytes < (4ll << 30)) budget_bytes = 4ll << 30;
  const int64_t budget_rows = std::max<int64_t>(budget_bytes / (24 * N + 4), 1);
  EstepWork &w = b->ew;
  if (w.N != N) {
    w.alpha.release();
    w.rows_cap = 0;
    w.N = N;
  }
  w.stats_base = dev_stats;
  {
    // per-wave slots of k_estep_accum: one workgroup per CU at most (its LDS holds four histograms), within 1 GB
    const int64_t slot_bytes = stats_size(NP, m->R) * (int64_t)sizeof(double);
    w.seq_blocks = (int)std::max<int64_t>(16, std::min<int64_t>(256, ((int64_t)1 << 30) / (4 * slot_bytes)));
  }
  IntervalTab iv;
  EmisTab em;
  fill_tabs(m, b, iv, em, ratio);     // fit applies the ratios to emissions too (basehmm.py:510)
  size_t pos_in_order = 0;
  while (pos_in_order < (size_t)b->n) {
    // next group: consecutive slots of the longest-first order
    std::vector<int> g_order;
    std::vector<int64_t> grow0((size_t)b->n, 0);
    std::vector<int> chunk_iv;
    std::vector<int64_t> chunk_t0;
    int64_t rows = 0;
    while (pos_in_order < (size_t)b->n) {
      const int id = b->h_order[pos_in_order];
      const int64_t T = b->h_len[id];
      if (!g_order.empty() && rows + T > budget_rows) break;
      g_order.push_back(id);
      grow0[id] = rows;
      for (int64_t t0 = 0; t0 < T; t0 += kEstepChunk) {
        chunk_iv.push_back(id);
        chunk_t0.push_back(t0);
      }
      rows += T;
      ++pos_in_order;
    }
    if (rows == 0) continue;
    if (rows > w.rows_cap) {
      HIPCHK(w.alpha.alloc((size_t)rows * N + 1));
      HIPCHK(w.beta.alloc((size_t)rows * N + 1));
      HIPCHK(w.wrows.alloc((size_t)rows * N + 1));
      HIPCHK(w.escale.alloc((size_t)rows + 1));
      w.rows_cap = rows;
    }
    if (b->n > w.n_cap) {
      HIPCHK(w.fwd_lp.alloc((size_t)b->n + 1));
      HIPCHK(w.dead.alloc((size_t)b->n + 1));
      w.n_cap = b->n;
    }
    HIPCHK(hipMemset(w.dead.p, 0, (size_t)(b->n + 1) * sizeof(int)));
    HIPCHK(hipMemset(w.escale.p, 0, ((size_t)rows + 1) * sizeof(int)));
    HIPCHK(w.order.upload(g_order.data(), g_order.size()));
    HIPCHK(w.grow0.upload(grow0.data(), grow0.size()));
    HIPCHK(w.chunk_iv.upload(chunk_iv.data(), chunk_iv.size()));
    HIPCHK(w.chunk_t0.upload(chunk_t0.data(), chunk_t0.size()));
    IntervalTab giv = iv;
    giv.order = w.order.p;
    giv.out0 = w.grow0.p;
    const int n_iv = (int)g_order.size(), n_chunks = (int)chunk_iv.size();
    HIPCHK(w.part_seq.ensure((size_t)std::max(1, std::min(w.seq_blocks, (n_chunks + 3) / 4)) * 4 * (size_t)stats_size(NP, m->R)));
    nt_dispatch(m->NP, [&](auto nt) { launch_estep<nt>(m, giv, em, ratio, n_iv, n_chunks, w, b->ratios.p, b->sP); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->sP));
    if (int rc = estep_results(b, w.fwd_lp.p, w.dead.p, &g_order, lp_out, dead_out)) return rc;
  }
  return TEHMM_OK;
}

// ---- chunk-parallel E-step on the fused posterior passes (tehmm_estep.hip.h) -----------------------------
// Track partition of the reduction kernels (tehmm_estep.hip.h): tracks of at most TEHMM_ESTEP_SMALL rows are
// packed into 16-row tiles for the one-hot product on the matrix cores, the others into LDS histogram groups of
// at most `cap_rows` rows (first fit, decreasing).
// Where the split lies (measured, config-4 model, 50 Mb, reduce stage): tracks of <= 9 rows on the matrix cores
// 21.6 ms, <= 21 rows 17.2, <= 31 (all ten small tracks) 16.3 -- a 16-row tile costs 12 matrix instructions per
// 16-item tile and step (~9 ns per row and CU), a track in LDS ~190-270 ns (nine ds_add_f64 at ~1 lane per cycle,
// more when items share a symbol), and the LDS kernel's workgroups do not share a CU with the 416-register waves
// of the one-hot kernel, so the two add up rather than overlap: break-even near 40 rows.
// TEHMM_ESTEP_SMALL overrides (largest track, in rows, that takes the one-hot product): EvalKnobs::estep_small.
static void estep_build_groups(const tehmm_model *m, int cap_rows, int small, EstepGroups &eg) {
  std::memset(&eg, 0, sizeof(eg));
  std::vector<int> big;
  int row = 0;
  for (int i = 0; i < TEHMM_ESTEP_MAXRT * 16; ++i) eg.rt_info[i] = -1;
  for (int k = 0; k < m->K; ++k) {
    if (m->rowcnt[k] <= small && row + m->rowcnt[k] <= TEHMM_ESTEP_MAXRT * 16) row = fill_track_rows(m, k, row, eg.rt_info, eg.rt_grow);
    else big.push_back(k);
  }
  eg.n_rt = (row + 15) / 16;
  std::stable_sort(big.begin(), big.end(), [&](int a, int b2) { return m->rowcnt[a] > m->rowcnt[b2]; });
  std::vector<std::vector<int>> bins;
  std::vector<int> load;
  for (int k : big) {
    size_t g = 0;
    while (g < bins.size() && load[g] + m->rowcnt[k] > cap_rows) ++g;
    if (g == bins.size()) { bins.emplace_back(); load.push_back(0); }
    bins[g].push_back(k);
    load[g] += m->rowcnt[k];
  }
  int slot = 0;
  eg.n_lds = (int)bins.size();
  for (size_t g = 0; g < bins.size(); ++g) {
    eg.first[g] = slot;
    int lrow = 0;
    for (int k : bins[g]) {
      eg.info[slot] = (k & 127) | ((m->rowcnt[k] & 511) << 7) | (lrow << 16);
      eg.gbase[slot] = m->rowbase[k];
      lrow += m->rowcnt[k];
      ++slot;
    }
    eg.rows[g] = lrow;
  }
  eg.first[bins.size()] = slot;
}

static bool estep_fused_wanted(const tehmm_model *m, const tehmm_batch *b, bool ratio, const EvalKnobs &kn) {
  const int CS = kn.spec_chunk;
  if (!kn.estep_fused) return false;
  if (ratio || m->N >= 64 || m->NP > 64 || CS <= 0 || b->total < 2 * (int64_t)CS) return false;
  if (!m->ptab.p || m->K > 78 || m->K > 127) return false;
  for (int k = 0; k < m->K; ++k)
    if (m->rowcnt[k] > 511) return false;
  return true;
}

template <int NT>
static int launch_estep_reduce(tehmm_batch *b, const tehmm_model *m, const IntervalTab &iv, double *dev_stats,
                               hipStream_t st) {
  LaneWork &lw = b->lw;
  EstepWork &w = b->ew;
  const LaneGeom lg = lane_geom(lw);
  const EstepGroups &eg = w.h_groups;
  const int64_t n_tiles = (int64_t)lw.n_groups * 4;
  double *gC = dev_stats + stats_off_C(m->NP), *gstart = dev_stats + stats_off_start(),
         *gstat = dev_stats + stats_off_stat(m->NP);
  // the three reductions are independent: the LDS-atomic histograms (LDS pipe) run next to the two matrix-core
  // products on their own streams.  Every writer owns a slot of a partial buffer; the fold kernels add the slots in
  // order (tehmm_estep.hip.h: reproducible sums).
  (void)hipEventRecord(b->evX[kEvxFork], st);
  const int gxm = (int)std::max<int64_t>(1, std::min<int64_t>((n_tiles + 3) / 4, 512));
  const int cells_xi = NT * NT + NT;
  HIPCHK(w.part_xi.ensure((size_t)gxm * 4 * cells_xi));
  int gx = 0, gxh = 0, max_rows = 0, tot_rows = 0;
  if (eg.n_lds > 0) {
    for (int g = 0; g < eg.n_lds; ++g) { max_rows = std::max(max_rows, eg.rows[g]); tot_rows += eg.rows[g]; }
    const size_t lds = (size_t)max_rows * NT * sizeof(double) + (size_t)m->K * sizeof(int) + 16;
    allow_lds(k_estep_hist_lds<NT>, lds);
    gx = (int)std::max<int64_t>(1, std::min<int64_t>((n_tiles + 7) / 8, 256));
    HIPCHK(w.part_lds.ensure((size_t)gx * tot_rows * NT));
    const int shift = hist_fixed_point_shift((double)hist_positions_per_wg(n_tiles, gx, lw.L));
    (void)hipStreamWaitEvent(b->sV, b->evX[kEvxFork], 0);
    hipLaunchKernelGGL((k_estep_hist_lds<NT>), dim3(gx, eg.n_lds), dim3(512), lds, b->sV, iv, lg,
                       (const EstepGroups *)w.d_groups.p, m->N, b->KP, (const uint8_t *)b->obs.p,
                       (const float *)lw.GAM32.p, w.part_lds.p, shift);
    hipLaunchKernelGGL(k_estep_fold_lds, dim3((max_rows * NT + 255) / 256, eg.n_lds), dim3(256), 0, b->sV,
                       (const double *)w.part_lds.p, gx, m->N, NT, (const EstepGroups *)w.d_groups.p, gstat);
    (void)hipEventRecord(b->ev[kEvLdsDone], b->sV);
  }
  if (eg.n_rt > 0) {
    constexpr int RTG = EstepGeom<NT>::RTG;
    (void)hipStreamWaitEvent(b->sB, b->evX[kEvxFork], 0);
    gxh = (int)std::max<int64_t>(1, std::min<int64_t>(n_tiles, 768));     // one tile per workgroup at a time, 3 per CU
    HIPCHK(w.part_rt.ensure((size_t)gxh * eg.n_rt * 16 * NT));
    hipLaunchKernelGGL((k_estep_hist_mfma<NT>), dim3(gxh, (eg.n_rt + RTG - 1) / RTG), dim3(TEHMM_ESTEP_HW * 64), 0, b->sB, iv, lg,
                       (const EstepGroups *)w.d_groups.p, m->N, b->KP, (const uint8_t *)b->obs.p,
                       (const float *)lw.GAM32.p, w.part_rt.p);
    hipLaunchKernelGGL(k_estep_fold_rows, dim3((eg.n_rt * 16 * NT + 255) / 256), dim3(256), 0, b->sB,
                       (const double *)w.part_rt.p, gxh, m->N, NT, (const EstepGroups *)w.d_groups.p, gstat);
    (void)hipEventRecord(b->evX[kEvxRowsDone], b->sB);
  }
  hipLaunchKernelGGL((k_estep_xi<NT>), dim3(gxm), dim3(256), 0, st, iv, lg, m->N, (const float *)lw.AL32.p,
                     (const float *)lw.GAM32.p, (const float *)lw.WZ32.p, w.part_xi.p);
  hipLaunchKernelGGL(k_estep_fold_xi, dim3((cells_xi + 255) / 256), dim3(256), 0, st, (const double *)w.part_xi.p, gxm * 4,
                     m->N, NT, gC, gstart);
  if (eg.n_lds > 0) (void)hipStreamWaitEvent(st, b->ev[kEvLdsDone], 0);
  if (eg.n_rt > 0) (void)hipStreamWaitEvent(st, b->evX[kEvxRowsDone], 0);
  return TEHMM_OK;
}

static EstepOutcome estep_fused(tehmm_model_t *m, tehmm_batch_t *b, const EvalKnobs &kn, double *dev_stats, double *lp_out,
                                int *dead_out) {
  b->lw.rix_ref = kn.rowindex_ref;
  const int CS = kn.spec_chunk;
  if (!estep_fused_wanted(m, b, false, kn)) return EstepOutcome::Declined;
  const int LS = lane_sub_size(CS, b->total, kn.lane_sub);
  if (LS <= 0) return EstepOutcome::Declined;
  LaneWork &lw = b->lw;
  EstepWork &w = b->ew;
  if (!(lw.AL32.p && lw.GAM32.p && lw.L == LS && lw.CS == CS && lw.NP == m->NP)) {
    // three float rows + index records per position must fit; otherwise the grouped sequential path
    size_t free_b = 0, total_b = 0;
    HIPCHK(dev_mem_info(&free_b, &total_b));
    const double per = (double)b->total * (3.0 * 32.0 * al32_pairs(m->NP) + 40.0) * 1.15;
    if (per > 0.85 * (double)free_b) return EstepOutcome::Declined;
  }
  if (int rc = spec_prepare(b, m, CS)) return rc;
  if (int rc = lane_prepare(b, m, CS, LS, true, false, false, true, false)) return rc;
  const size_t na = (size_t)std::max(1, lw.n_groups) * LS * 512 * al32_pairs(m->NP);
  if (!lw.GAM32.p) {
    HIPCHK(lw.GAM32.alloc(na));
    HIPCHK(lw.WZ32.alloc(na));
    HIPCHK(hipMemset(lw.GAM32.p, 0, na * sizeof(float)));      // (slots beyond an interval's end are read, never written)
    HIPCHK(hipMemset(lw.WZ32.p, 0, na * sizeof(float)));
  }
  if (int rc = ensure_interval_scalars(b)) return rc;
  if (w.groups_model != m->uid || !w.d_groups.p) {
    const int cap_rows = (int)((160 * 1024 - (size_t)m->K * sizeof(int) - 64) / ((size_t)m->NP * sizeof(double)));
    estep_build_groups(m, cap_rows, kn.estep_small, w.h_groups);
    HIPCHK(w.d_groups.upload(&w.h_groups, 1));
    w.groups_model = m->uid;
  }
  IntervalTab iv;
  EmisTab em;
  fill_tabs(m, b, iv, em, false);
  SpecWork &sw = b->sw;
  int WuF = 64;
  if (int rc = fb_warmup(b, m, LS, iv, without_lds_tables(em), kn, &WuF)) return rc;
  const FbChunks fc = fb_chunks(sw, lw, CS);
  hipStream_t st = b->sP;
  reset_timings(b);
  (void)hipEventRecord(b->ev[kEvStart], st);
  (void)hipMemsetAsync(b->dead.p, 0, (size_t)(b->n + 1) * sizeof(int), st);
  (void)hipMemsetAsync(sw.stats.p + 2, 0, 4 * sizeof(int), st);
  int rc = TEHMM_OK;
  const bool tail = fused_tail_runs(m, kn.fused_tail);
  nt_dispatch(m->NP, [&](auto nt) {
    rc = launch_fused_fb<nt>(b, m, iv, em, fc, WuF, st, b->ev[kEvFwdEnd], b->ev[kEvBwdEnd], tail, true);
  });
  if (rc) return rc;
  (void)hipEventRecord(b->ev[kEvFusedChainEnd], st);
  nt_dispatch(m->NP, [&](auto nt) { rc = launch_estep_reduce<nt>(b, m, iv, dev_stats, st); });
  if (rc) return rc;
  (void)hipEventRecord(b->ev[kEvFusedReduceEnd], st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  add_stage(b, "estep_forward_pass", kEvStart, kEvFwdEnd);
  add_stage(b, "estep_backward_pass", kEvFwdEnd, kEvBwdEnd);
  add_stage(b, "estep_backward_chain", kEvBwdEnd, kEvFusedChainEnd);
  add_stage(b, "estep_reduce", kEvFusedChainEnd, kEvFusedReduceEnd);
  stage_times(b);
  if ((rc = add_chain_counters(b))) return rc;
  // (only where the knob is set: callers compare the timing list of a fused E-step name by name, in order)
  if (kn.fused_tail_set) add_counter(b, "count:fused_tail", tail ? 1 : 0);
  if ((rc = estep_results(b, b->fwd_lp.p, b->dead.p, nullptr, lp_out, dead_out))) return rc;
  return EstepOutcome::Ran;
}

// ---- E-step on the item-parallel passes of tehmm_wide.hip.h (tehmm_wide_estep.hip.h): 64 <= N <= 128 states, and
// segment ratios at any N <= 128 ---------------------------------------------------------------------------------
static bool estep_wide_wanted(const tehmm_model *m, const tehmm_batch *b, bool ratio, const EvalKnobs &kn) {
  const int mode = kn.estep_wide;                   // 0: off, 1: where the fused passes do not apply, 2: everywhere
  if (mode == 0 || m->N > 128 || b->total < 1024) return false;
  if (mode == 1 && !(ratio || m->N >= 64)) return false;
  if (m->K > 255) return false;
  return true;
}

// Track partition of the wide reductions: tracks of more than `small` rows whose histogram [rows][NPW or NPW / 2]
// fits a CU's LDS go there (w.h_lds, w.lds_nsplit), the others (and START / DIAG) through the one-hot product
// (w.h_rows).  False: more rows than the row table holds.
static bool wide_estep_build_rows(const tehmm_model *m, int NPW, int small, WideWork &w) {
  WideRows &wr = w.h_rows;
  WideLds &wl = w.h_lds;
  std::memset(&wl, 0, sizeof(wl));
  for (int i = 0; i < TEHMM_ESTEP_MAXRT * 16; ++i) { wr.info[i] = -1; wr.grow[i] = 0; }
  constexpr size_t kLdsCap = 150 * 1024;
  int big_rows = 0;
  for (int k = 0; k < m->K; ++k)
    if (m->rowcnt[k] > small) big_rows = std::max(big_rows, m->rowcnt[k]);
  w.lds_nsplit = (size_t)big_rows * NPW * 8 <= kLdsCap ? 1 : 2;
  int row = 0;
  wr.info[row++] = TEHMM_WIDE_ROW_START;
  wr.info[row++] = TEHMM_WIDE_ROW_DIAG;
  for (int k = 0; k < m->K; ++k) {
    if (m->rowcnt[k] > small && (size_t)m->rowcnt[k] * (NPW / w.lds_nsplit) * 8 <= kLdsCap) {
      wl.col[wl.n_trk] = k;
      wl.rows[wl.n_trk] = m->rowcnt[k];
      wl.gbase[wl.n_trk] = m->rowbase[k];
      ++wl.n_trk;
    } else {
      if (row + m->rowcnt[k] > TEHMM_ESTEP_MAXRT * 16) return false;
      row = fill_track_rows(m, k, row, wr.info, wr.grow);
    }
  }
  wr.n_rt = (row + 15) / 16;
  return true;
}

template <int NPW>
static int launch_wide_estep_reduce(tehmm_batch *b, const tehmm_model *m, const IntervalTab &iv, const LaneGeom &lg, bool ratio,
                                    const EvalKnobs &kn, double *dev_stats, hipStream_t st) {
  WideWork &w = b->ww;
  using G = WideEstepGeom<NPW>;
  const int64_t n_tiles = ((int64_t)w.n_items + 15) / 16;
  double *gC = dev_stats + stats_off_C(m->NP), *gD = dev_stats + stats_off_D(m->NP), *gstart = dev_stats + stats_off_start(),
         *gstat = dev_stats + stats_off_stat(m->NP);
  // work units = item tiles x SQ position ranges: at least ~4096 of them (a 2 Mb batch has 1000 item tiles; the GPU
  // 1024 SIMDs), ranges of 16 positions or more
  int SQ = 1;
  while (SQ < 8 && n_tiles * SQ < 4096 && w.L / (2 * SQ) >= 16 && w.L % (2 * SQ) == 0) SQ *= 2;
  if (kn.wide_estep_sq >= 1 && w.L % kn.wide_estep_sq == 0) SQ = kn.wide_estep_sq;
  const int64_t n_units = n_tiles * SQ;
  // xi: two workgroups per CU at most; gamma product: one unit per workgroup at a time, partial buffer <= 128 MB
  const int gxm = (int)std::max<int64_t>(1, std::min<int64_t>((n_units + G::TPW - 1) / G::TPW, 512));
  HIPCHK(w.part_xi.ensure((size_t)gxm * G::TPW * NPW * NPW));
  const int nrt = w.h_rows.n_rt;
  const int64_t slot_rows = (int64_t)nrt * 16 * NPW * 8;
  // gamma product: four units per workgroup at a time (one per wave), up to three row tiles per wave; partial buffer <= 128 MB
  const int rtw = std::min(nrt, NPW <= 64 ? 4 : 3);      // (every group of row tiles reads the gamma rows once more)
  const int gxr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((n_units + 3) / 4, 256), std::max<int64_t>(64, ((int64_t)32 << 20) / slot_rows)));
  HIPCHK(w.part_rows.ensure((size_t)gxr * 4 * nrt * 16 * NPW));
  // the products are independent: the gamma product and the LDS histograms run on their own streams next to the xi
  // product (TEHMM_WIDE_ESTEP_SERIAL=1: one after the other, for profiling)
  const bool serial = kn.wide_estep_serial;
  hipStream_t sB = serial ? st : b->sB, sV = serial ? st : b->sV;
  (void)hipEventRecord(b->evX[kEvxFork], st);
  (void)hipStreamWaitEvent(sB, b->evX[kEvxFork], 0);
  bool_dispatch(ratio, [&](auto r) {
    auto rows = [&](auto rt) {      // rt: row tiles per wave
      hipLaunchKernelGGL((k_wide_estep_rows<NPW, r, rt>), dim3(gxr, (nrt + rtw - 1) / rtw), dim3(256), 0, sB, iv, lg,
                         (const WideRows *)w.d_rows.p, b->KP, (const uint8_t *)b->obs.p,
                         (const double *)(r ? b->ratios.p : nullptr), (const float *)w.GAM.p, w.part_rows.p, SQ);
    };
    if constexpr (NPW <= 64) nt_dispatch_of<1, 2, 3, 4>(rtw, rows);
    else nt_dispatch_of<1, 2, 3>(rtw, rows);
  });
  hipLaunchKernelGGL(k_wide_fold_rows, dim3((nrt * 16 * m->N + 255) / 256), dim3(256), 0, sB, (const double *)w.part_rows.p,
                     gxr * 4, m->N, NPW, m->NP, (const WideRows *)w.d_rows.p, gstat, gstart, gD);
  (void)hipEventRecord(b->evX[kEvxRowsDone], sB);
  if (w.h_lds.n_trk > 0) {
    // tracks with many symbols: fixed-point histograms privatised in LDS, on a third stream
    const int nsplit = w.lds_nsplit, HS = NPW / nsplit;
    int max_rows = 0, tot_rows = 0;
    for (int t = 0; t < w.h_lds.n_trk; ++t) { max_rows = std::max(max_rows, w.h_lds.rows[t]); tot_rows += w.h_lds.rows[t]; }
    const size_t lds = (size_t)max_rows * HS * sizeof(unsigned long long);
    const int gxl = (int)std::max<int64_t>(1, std::min<int64_t>((n_units + 7) / 8, 256));
    HIPCHK(w.part_lds.ensure((size_t)gxl * tot_rows * NPW));
    // the largest sum one workgroup can reach in a cell: its positions (L / SQ per item and unit) x the largest ratio
    const double vmax = (double)hist_positions_per_wg(n_units, gxl, w.L / SQ) * (ratio ? std::max(1.0, w.ratio_max) : 1.0);
    const int shift = hist_fixed_point_shift(vmax);
    (void)hipStreamWaitEvent(sV, b->evX[kEvxFork], 0);
    bool_dispatch(ratio, [&](auto r) {
      nt_dispatch_of<1, 2>(nsplit, [&](auto ns) {      // ns: state ranges a track's histogram is split into
        allow_lds(k_wide_estep_hist_lds<NPW, ns, r>, lds);
        hipLaunchKernelGGL((k_wide_estep_hist_lds<NPW, ns, r>), dim3(gxl, w.h_lds.n_trk * nsplit), dim3(512), lds, sV, iv, lg,
                           (const WideLds *)w.d_lds.p, m->N, b->KP, (const uint8_t *)b->obs.p,
                           (const double *)(r ? b->ratios.p : nullptr), (const float *)w.GAM.p, w.part_lds.p, shift, SQ);
      });
    });
    hipLaunchKernelGGL(k_wide_fold_lds, dim3((max_rows * HS + 255) / 256, w.h_lds.n_trk * nsplit), dim3(256), 0, sV,
                       (const double *)w.part_lds.p, gxl, m->N, m->NP, HS, nsplit, (const WideLds *)w.d_lds.p, gstat);
    (void)hipEventRecord(b->ev[kEvLdsDone], sV);
  }
  hipLaunchKernelGGL((k_wide_estep_xi<NPW>), dim3(gxm), dim3(256), 0, st, iv, lg, (const float *)w.AL.p, (const float *)w.WZ.p,
                     w.part_xi.p, SQ);
  hipLaunchKernelGGL(k_wide_fold_xi, dim3((m->N * m->N + 255) / 256), dim3(256), 0, st, (const double *)w.part_xi.p, gxm * G::TPW,
                     m->N, NPW, m->NP, gC);
  (void)hipStreamWaitEvent(st, b->evX[kEvxRowsDone], 0);
  if (w.h_lds.n_trk > 0) (void)hipStreamWaitEvent(st, b->ev[kEvLdsDone], 0);
  return TEHMM_OK;
}

static EstepOutcome estep_wide(tehmm_model_t *m, tehmm_batch_t *b, const EvalKnobs &kn, bool ratio, double *dev_stats,
                               double *lp_out, int *dead_out) {
  if (!estep_wide_wanted(m, b, ratio, kn)) return EstepOutcome::Declined;
  const int NPW = wide_npw<TEHMM_WIDE_ESTEP_WIDTHS>(m->N);
  if (NPW <= 0) return EstepOutcome::Declined;
  WideWork &w = b->ww;
  if (!w.h_flags) HIPCHK(hipHostMalloc((void **)&w.h_flags, 64, hipHostMallocDefault));
  const int L = wide_item_length(b, kn);
  if (!(w.GAM.p && w.L == L && w.NPW == NPW)) {
    // emission rows + three float rows per position must fit
    size_t free_b = 0, total_b = 0;
    HIPCHK(dev_mem_info(&free_b, &total_b));
    if ((double)b->total * NPW * 22.0 + (double)(b->total / L + b->n + 64) * NPW * 40.0 > 0.85 * (double)free_b)
      return EstepOutcome::Declined;
  }
  bool fits = true;
  if (int rc = wide_geometry(b, NPW, L, &fits)) return rc;
  if (!fits) return EstepOutcome::Declined;
  const size_t na = (size_t)std::max(1, w.n_groups) * 64 * L * (NPW / 4) * 4;
  if (!w.GAM.p) {
    HIPCHK(w.GAM.alloc(na));
    HIPCHK(w.WZ.alloc(na));
    w.al_zeroed = false;
  }
  if (!w.al_zeroed) {       // slots no pass writes (beyond an item's end) are read by the reductions: zero once
    HIPCHK(hipMemset(w.AL.p, 0, na * sizeof(float)));
    HIPCHK(hipMemset(w.GAM.p, 0, na * sizeof(float)));
    HIPCHK(hipMemset(w.WZ.p, 0, na * sizeof(float)));
    w.al_zeroed = true;
  }
  if (int rc = ensure_interval_scalars(b)) return rc;
  if (w.rows_model != m->uid || w.rows_npw != NPW || !w.d_rows.p) {
    if (!wide_estep_build_rows(m, NPW, kn.estep_small, w)) return EstepOutcome::Declined;
    HIPCHK(w.d_rows.upload(&w.h_rows, 1));
    HIPCHK(w.d_lds.upload(&w.h_lds, 1));
    w.rows_model = m->uid;
    w.rows_npw = NPW;
  }
  if (ratio && w.h_lds.n_trk > 0 && w.ratio_max <= 0.0) {
    // the fixed-point scale of the LDS histograms needs the largest ratio of the batch (once per batch)
    if (!w.d_rmax.p) HIPCHK(w.d_rmax.alloc(1));
    HIPCHK(hipMemset(w.d_rmax.p, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_ratio_max, dim3(grid_for(b->total_pad, 256, 2048)), dim3(256), 0, b->sP, (const double *)b->ratios.p,
                       b->total_pad, w.d_rmax.p);
    unsigned long long bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, w.d_rmax.p, sizeof(bits), hipMemcpyDeviceToHost, b->sP));
    HIPCHK(hipStreamSynchronize(b->sP));
    double rmax = 0.0;
    std::memcpy(&rmax, &bits, sizeof(rmax));
    if (!(rmax < 1e12)) return EstepOutcome::Declined;      // (inf / NaN ratios: the sequential kernels own their semantics)
    w.ratio_max = std::max(rmax, 1e-300);
  }
  IntervalTab iv;
  EmisTab em;
  fill_tabs(m, b, iv, em, ratio);     // fit applies the ratios to emissions too (basehmm.py:510)
  const LaneGeom lg = wide_lane_geom(w);
  hipStream_t st = b->sP;
  reset_timings(b);
  (void)hipEventRecord(b->ev[kEvStart], st);
  HIPCHK(hipMemsetAsync(w.flags.p, 0, 4 * sizeof(int), st));
  launch_wide_emis(b, m, iv, em, lg, ratio ? 3 : 2, nullptr, st);
  (void)hipEventRecord(b->ev[kEvWideEmisEnd], st);
  (void)hipEventRecord(b->ev[kEvWideAttempt], st);
  if (int rc = wide_post_attempt(b, m, iv, kn, wide_first_warmup(w, m, kn, false), st, b->ev[kEvFwdEnd], true)) return rc;
  WideRetries re = {b->ev[kEvWideAttempt], b->ev[kEvBwdEnd], 1};
  bool verified = false;
  if (int rc = wide_verdict(b, m, iv, kn, st, b->ev[kEvFwdEnd], true, &re, &verified)) return rc;
  if (!verified) return EstepOutcome::Declined;      // impossible rows, or links that do not verify
  int rc = TEHMM_OK;
  nt_dispatch_of<TEHMM_WIDE_ESTEP_WIDTHS>(NPW, [&](auto npw) { rc = launch_wide_estep_reduce<npw>(b, m, iv, lg, ratio, kn, dev_stats, st); });
  if (rc) return rc;
  (void)hipEventRecord(b->ev[kEvWideReduceEnd], st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  add_stage(b, "estep_emission_rows", kEvStart, kEvWideEmisEnd);
  add_stage(b, "estep_forward_pass", kEvWideAttempt, kEvFwdEnd);      // (forward / backward: of the LAST attempt)
  add_stage(b, "estep_backward_pass", kEvFwdEnd, kEvBwdEnd);
  add_stage(b, "estep_reduce", kEvBwdEnd, kEvWideReduceEnd);
  stage_times(b);
  add_counter(b, "count:wide_estep_attempts", (double)re.attempts);
  add_counter(b, "count:wide_estep_warmup", (double)w.wu_ok);
  if ((rc = estep_results(b, b->fwd_lp.p, nullptr, nullptr, lp_out, dead_out))) return rc;
  return EstepOutcome::Ran;
}

// Raw statistics of every interval of the batch ADDED into dev_stats (device buffer of
// stats_size(NP, R) doubles, layout in tehmm_aux.hip.h); *dead_any: some interval met an impossible row
// after its first emittable one (the reference's lattices are NaN there).
static int estep_accumulate(tehmm_model_t *m, tehmm_batch_t *b, int use_ratios, double *dev_stats, double *lp_out,
                            int *dead_out) {
#ifdef TEHMM_DEV_NT
  if (m->N < 64 && m->NP != TEHMM_DEV_NT)
    return fail(TEHMM_ERR_UNSUPPORTED, "development build: fused kernels exist for one padded state count only");
#endif
  *lp_out = 0.0;
  *dead_out = 0;
  b->h_fwd_lp.assign((size_t)b->n, 0.0);
  if (b->n == 0 || b->total == 0) return TEHMM_OK;
  const bool ratio = use_ratios && b->has_ratios;
  const EvalKnobs kn = read_eval_knobs();
  // the routes in order; each one declines what it does not take
  if (!ratio && m->N < 64 && kn.estep_wide != 2) {
    const EstepOutcome o = estep_fused(m, b, kn, dev_stats, lp_out, dead_out);
    if (o.kind != EstepOutcome::Declined) return o.rc;
  }
  const EstepOutcome o = estep_wide(m, b, kn, ratio, dev_stats, lp_out, dead_out);
  if (o.kind != EstepOutcome::Declined) return o.rc;
  if (m->N >= 64)
    return fail(TEHMM_ERR_UNSUPPORTED, "E-step at N >= 64: the item-parallel passes do not apply to this batch (impossible "
                                       "emission rows, links that do not verify, or a batch below 1024 rows): use the array-level path");
  return estep_sequential(m, b, ratio, dev_stats, lp_out, dead_out);
}

int64_t tehmm_model_stats_size(const tehmm_model_t *m) {
  if (m && m->large) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_model_stats_size: no device-resident statistics for N > 128");
  return m ? stats_size(m->NP, m->R) : 0;
}

int tehmm_estep_batch_device(tehmm_model_t *m, tehmm_batch_t *b, int use_ratios, double *dev_stats,
                             double *logprob_sum) {
  if (!m || !b || !dev_stats || !logprob_sum)
    return fail(TEHMM_ERR_ARG, "tehmm_estep_batch_device: NULL argument");
  if (m->K != b->K) return fail(TEHMM_ERR_ARG, "tehmm_estep_batch_device: model/batch track count differ");
  if (m->N > 128)
    return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_estep_batch_device: N > 128 (the E-step of such a model runs on the "
                                       "array-level entry points)");
  double lp = 0.0;
  int dead = 0;
  int rc = estep_accumulate(m, b, use_ratios, dev_stats, &lp, &dead);
  if (rc) return rc;
  const double nan = std::nan("");
  // slots 0 / 1 of the buffer: log-likelihood sum (NaN poisons it, as the reference's NaN lattices would)
  // and sequence count -- they travel with the statistics through the all-reduce
  double head[2];
  HIPCHK(hipMemcpy(head, dev_stats, sizeof(head), hipMemcpyDeviceToHost));
  head[0] += dead ? nan : lp;
  head[1] += (double)b->n;
  HIPCHK(hipMemcpy(dev_stats, head, sizeof(head), hipMemcpyHostToDevice));
  if (dead) {      // the reference's statistics are NaN from such a sequence on: poison the buffer
    std::vector<double> bad((size_t)stats_size(m->NP, m->R), nan);
    bad[1] = head[1];
    HIPCHK(hipMemcpy(dev_stats, bad.data(), bad.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  *logprob_sum = dead ? nan : lp;
  return TEHMM_OK;
}

int tehmm_estep_batch(tehmm_model_t *m, tehmm_batch_t *b, int use_ratios, double *start,
                      double *trans, double *obsStats, double *logprob_sum) {
  if (!m || !b || !start || !trans || !obsStats || !logprob_sum)
    return fail(TEHMM_ERR_ARG, "tehmm_estep_batch: NULL argument");
  if (m->K != b->K) return fail(TEHMM_ERR_ARG, "tehmm_estep_batch: model/batch track count differ");
  if (m->N > 128)
    return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_estep_batch: N > 128 (the E-step of such a model runs on the array-level "
                                       "entry points)");
  *logprob_sum = 0.0;
  if (b->n == 0 || b->total == 0) return TEHMM_OK;
  const int N = m->N, NP = m->NP, K = m->K, S = m->S;
  EstepWork &w = b->ew;
  const size_t ssz = (size_t)stats_size(NP, m->R);
  HIPCHK(w.statbuf.ensure(ssz));
  HIPCHK(hipMemset(w.statbuf.p, 0, ssz * sizeof(double)));
  double lp_total = 0.0;
  int dead_any = 0;
  int rc = estep_accumulate(m, b, use_ratios, w.statbuf.p, &lp_total, &dead_any);
  if (rc) return rc;
  std::vector<double> hs(ssz);
  HIPCHK(hipMemcpy(hs.data(), w.statbuf.p, ssz * sizeof(double), hipMemcpyDeviceToHost));
  const double *hS = hs.data() + stats_off_start(), *hC = hs.data() + stats_off_C(NP),
               *hD = hs.data() + stats_off_D(NP), *hst = hs.data() + stats_off_stat(NP);
  const double nan = std::nan("");
  const double invN = 1.0 / (double)N;
  for (int i = 0; i < N; ++i) {
    start[i] += dead_any ? nan : hS[i];
    for (int j = 0; j < N; ++j) {
      double v = std::exp(m->h_lt[(size_t)i * N + j]) * hC[(size_t)i * NP + j];
      if (i == j) v += hD[i];
      trans[(size_t)i * N + j] += dead_any ? nan : v * invN;
    }
  }
  for (int k = 0; k < K; ++k)
    for (int s2 = 0; s2 < m->rowcnt[k]; ++s2)
      for (int j = 0; j < N; ++j)
        obsStats[((size_t)k * N + j) * S + s2] += dead_any ? nan : hst[(size_t)(m->rowbase[k] + s2) * NP + j];
  *logprob_sum = dead_any ? nan : lp_total;
  return TEHMM_OK;
}
