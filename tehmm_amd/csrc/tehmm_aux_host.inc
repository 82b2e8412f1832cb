// tehmm_aux_host.inc -- host side of the kernels in tehmm_aux.hip.h (included by tehmm_hip.hip):
// segment compression / mask compaction of track tables and the device-resident M-step.

// ---- TrackTable.segment / setMaskTable (track.py:449-533, 594-662) -------------------------------
int tehmm_segment_table_u8(int64_t T, int K, const uint8_t *data, int64_t n_seg, const int64_t *segOffsets,
                           const uint8_t *is_gaussian, const double *mapback, uint8_t *out, double *means) {
  if (T <= 0 || K <= 0 || K > TEHMM_MAX_TRACKS || n_seg <= 0 || !data || !segOffsets || !is_gaussian || !out || !means)
    return fail(TEHMM_ERR_ARG, "tehmm_segment_table_u8: bad argument");
  bool any_gauss = false;
  for (int k = 0; k < K; ++k) any_gauss = any_gauss || is_gaussian[k] != 0;
  if (any_gauss && !mapback) return fail(TEHMM_ERR_ARG, "tehmm_segment_table_u8: gaussian track without a map-back table");
  for (int64_t i = 0; i < n_seg; ++i)
    if (segOffsets[i] < 0 || segOffsets[i] >= T || (i > 0 && segOffsets[i] <= segOffsets[i - 1]))
      return fail(TEHMM_ERR_ARG, "tehmm_segment_table_u8: segment offsets must be ascending and inside the table");
  DBuf<uint8_t> d_data, d_g, d_out;
  DBuf<int64_t> d_off;
  DBuf<double> d_mb, d_means;
  HIPCHK(d_data.upload(data, (size_t)T * K));
  HIPCHK(d_off.upload(segOffsets, (size_t)n_seg));
  HIPCHK(d_g.upload(is_gaussian, (size_t)K));
  if (mapback) HIPCHK(d_mb.upload(mapback, (size_t)K * 256));
  HIPCHK(d_out.alloc((size_t)n_seg * K));
  HIPCHK(d_means.alloc((size_t)n_seg * K));
  hipLaunchKernelGGL(k_segment_table, dim3(grid_for(n_seg, 4, 16384)), dim3(256), 0, 0, T, K,
                     (const uint8_t *)d_data.p, n_seg, (const int64_t *)d_off.p, (const uint8_t *)d_g.p,
                     (const double *)d_mb.p, d_out.p, d_means.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d_out.p, (size_t)n_seg * K, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(means, d_means.p, (size_t)n_seg * K * sizeof(double), hipMemcpyDeviceToHost));
  return TEHMM_OK;
}

int tehmm_mask_table_u8(int64_t T, int K, const uint8_t *data, int KM, const uint8_t *maskdata, uint8_t *keep,
                        int32_t *run_full, uint8_t *out_data, int32_t *run_masked, int64_t *n_keep) {
  if (T <= 0 || K <= 0 || KM <= 0 || !data || !maskdata || !keep || !run_full || !out_data || !run_masked || !n_keep)
    return fail(TEHMM_ERR_ARG, "tehmm_mask_table_u8: bad argument");
  if (T > 0x7fffffffll) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_mask_table_u8: table longer than 2^31 - 1 rows");
  const int64_t nb = (T + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  DBuf<uint8_t> d_data, d_mask, d_keep, d_out;
  DBuf<unsigned> d_blk;
  DBuf<int32_t> d_rf, d_rm;
  DBuf<int64_t> d_tot;
  HIPCHK(d_data.upload(data, (size_t)T * K));
  HIPCHK(d_mask.upload(maskdata, (size_t)T * KM));
  HIPCHK(d_keep.alloc((size_t)T));
  HIPCHK(d_out.alloc((size_t)T * K));
  HIPCHK(d_blk.alloc((size_t)nb));
  HIPCHK(d_rf.alloc((size_t)T));
  HIPCHK(d_rm.alloc((size_t)T));
  HIPCHK(d_tot.alloc(1));
  hipLaunchKernelGGL(k_mask_flags, dim3((unsigned)nb), dim3(256), 0, 0, T, KM, (const uint8_t *)d_mask.p, d_keep.p,
                     d_blk.p);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, 0, nb, d_blk.p, d_tot.p);
  hipLaunchKernelGGL(k_mask_scatter, dim3((unsigned)nb), dim3(256), 0, 0, T, K, (const uint8_t *)d_data.p,
                     (const uint8_t *)d_keep.p, (const unsigned *)d_blk.p, d_rf.p, d_out.p, d_rm.p);
  HIPCHK(hipGetLastError());
  int64_t cut = 0;
  HIPCHK(hipMemcpy(&cut, d_tot.p, sizeof(cut), hipMemcpyDeviceToHost));
  const int64_t nk = T - cut;
  *n_keep = nk;
  HIPCHK(hipMemcpy(keep, d_keep.p, (size_t)T, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(run_full, d_rf.p, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (nk > 0) {
    HIPCHK(hipMemcpy(out_data, d_out.p, (size_t)nk * K, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(run_masked, d_rm.p, (size_t)nk * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return TEHMM_OK;
}

// ---- device-resident Baum-Welch: statistics buffers and the M-step --------------------------------
int tehmm_stats_alloc(const tehmm_model_t *m, double **dev_stats) {
  if (!m || !dev_stats) return fail(TEHMM_ERR_ARG, "tehmm_stats_alloc: bad argument");
  if (m->large) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_stats_alloc: no device-resident statistics for N > 128");
  *dev_stats = nullptr;
  HIPCHK(hipMalloc((void **)dev_stats, (size_t)stats_size(m->NP, m->R) * sizeof(double)));
  HIPCHK(hipMemset(*dev_stats, 0, (size_t)stats_size(m->NP, m->R) * sizeof(double)));
  return TEHMM_OK;
}
int tehmm_stats_zero(const tehmm_model_t *m, double *dev_stats) {
  if (!m || !dev_stats) return fail(TEHMM_ERR_ARG, "tehmm_stats_zero: bad argument");
  if (m->large) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_stats_zero: no device-resident statistics for N > 128");
  HIPCHK(hipMemset(dev_stats, 0, (size_t)stats_size(m->NP, m->R) * sizeof(double)));
  return TEHMM_OK;
}
int tehmm_stats_free(double *dev_stats) {
  if (dev_stats) HIPCHK(hipFree(dev_stats));
  return TEHMM_OK;
}
int tehmm_stats_head(const double *dev_stats, double *logprob_sum, double *nobs) {
  if (!dev_stats) return fail(TEHMM_ERR_ARG, "tehmm_stats_head: bad argument");
  double head[2];
  HIPCHK(hipMemcpy(head, dev_stats, sizeof(head), hipMemcpyDeviceToHost));
  if (logprob_sum) *logprob_sum = head[0];
  if (nobs) *nobs = head[1];
  return TEHMM_OK;
}

int tehmm_stats_copy(const tehmm_model_t *m, double *dev_stats, double *host_buf, int to_device) {
  if (!m || !dev_stats || !host_buf) return fail(TEHMM_ERR_ARG, "tehmm_stats_copy: bad argument");
  if (m->large) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_stats_copy: no device-resident statistics for N > 128");
  const size_t bytes = (size_t)stats_size(m->NP, m->R) * sizeof(double);
  if (to_device) HIPCHK(hipMemcpy(dev_stats, host_buf, bytes, hipMemcpyHostToDevice));
  else HIPCHK(hipMemcpy(host_buf, dev_stats, bytes, hipMemcpyDeviceToHost));
  return TEHMM_OK;
}

static MstepTracks mstep_tracks(const tehmm_model *m) {
  MstepTracks tr;
  tr.K = m->K;
  std::memcpy(tr.rowbase, m->rowbase, sizeof(tr.rowbase));
  std::memcpy(tr.rowcnt, m->rowcnt, sizeof(tr.rowcnt));
  return tr;
}

// every copy derived from tab (emission) / lt (trans) that the M-step or a constraint rewrote
static int mstep_rebuild(tehmm_model *m, const MstepTracks &tr, bool emission, bool trans) {
  const int N = m->N, NP = m->NP;
  if (emission) {
    if (int rcp = build_ptab(m)) return rcp;
    if (m->lds_rows > 0) {
      DBuf<int> d_lb;
      HIPCHK(d_lb.upload(m->ldsbase, (size_t)m->K));
      hipLaunchKernelGGL(k_model_ltab, dim3(m->K), dim3(256), 0, 0, tr, (const int *)d_lb.p, NP,
                         (const double *)m->tab.p, m->ltab.p);
      HIPCHK(hipDeviceSynchronize());
    }
  }
  if (trans) {
    hipLaunchKernelGGL(k_model_layouts, dim3(grid_for((int64_t)NP * NP, 256)), dim3(256), 0, 0, NP,
                       (const double *)m->lt.p, m->ltT.p, m->A.p, m->AT.p, m->ltG.p, m->AG.p, m->ATG.p, m->ltP.p);
    // host copy of the log-transition matrix (binade tables of the exact Viterbi, E-step transform)
    std::vector<double> hlt((size_t)NP * NP);
    HIPCHK(hipMemcpy(hlt.data(), m->lt.p, hlt.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) m->h_lt[(size_t)i * N + j] = hlt[(size_t)i * NP + j];
  }
  return TEHMM_OK;
}

int tehmm_model_mstep(tehmm_model_t *m, const double *dev_stats, int update_start, int update_trans,
                      int update_emission, double startprob_prior, double transmat_prior, double fudge,
                      int n_gauss, const int32_t *gauss_tracks, const double *gauss_values, double uniform_mix,
                      double *gauss_params) {
  if (!m || !dev_stats || n_gauss < 0 || (n_gauss > 0 && (!gauss_tracks || !gauss_values)))
    return fail(TEHMM_ERR_ARG, "tehmm_model_mstep: bad argument");
  if (m->N > 128) return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_model_mstep: N > 128 (no device-resident M-step)");
  for (int g = 0; g < n_gauss; ++g)
    if (gauss_tracks[g] < 0 || gauss_tracks[g] >= m->K)
      return fail(TEHMM_ERR_ARG, "tehmm_model_mstep: gaussian track index out of range");
  const int N = m->N, NP = m->NP;
  const MstepTracks tr = mstep_tracks(m);
  const size_t n_tab = (size_t)(m->R + 1) * NP;
  // (transMatEpsilons alone launches no constraint kernel: nothing can raise the status word, nothing to put back)
  const bool forced = m->c_trans || m->c_start || m->c_emis;
  if (forced) {
    // what a failed constraint puts back (device to device, in stream order: no synchronisation)
    HIPCHK(hipMemcpyAsync(m->c_save.p, m->lt.p, (size_t)NP * NP * sizeof(double), hipMemcpyDeviceToDevice, 0));
    HIPCHK(hipMemcpyAsync(m->c_save.p + (size_t)NP * NP, m->pi.p, (size_t)NP * sizeof(double),
                          hipMemcpyDeviceToDevice, 0));
    HIPCHK(hipMemcpyAsync(m->c_save.p + (size_t)NP * NP + NP, m->tab.p, n_tab * sizeof(double),
                          hipMemcpyDeviceToDevice, 0));
    HIPCHK(hipMemsetAsync(m->c_status.p, 0, sizeof(int), 0));
  }
  if (update_start || update_trans)
    hipLaunchKernelGGL(k_mstep_trans, dim3(1), dim3(128), 0, 0, N, NP, dev_stats, update_start, update_trans,
                       startprob_prior, transmat_prior, m->lt.p, m->pi.p, m->c_eps ? 1 : 0);
  if (update_emission) {
    hipLaunchKernelGGL(k_mstep_emis, dim3(grid_for((int64_t)m->K * N, 64)), dim3(64), 0, 0, tr, N, NP, dev_stats,
                       fudge, m->tab.p);
    if (n_gauss > 0) {
      DBuf<int> d_gt;
      DBuf<double> d_val, d_gp;
      HIPCHK(d_gt.upload(gauss_tracks, (size_t)n_gauss));
      HIPCHK(d_val.upload(gauss_values, (size_t)n_gauss * m->S));
      HIPCHK(d_gp.alloc((size_t)n_gauss * N * 2));
      hipLaunchKernelGGL(k_mstep_gauss, dim3(grid_for((int64_t)n_gauss * N, 64)), dim3(64), 0, 0, tr, n_gauss,
                         (const int *)d_gt.p, (const double *)d_val.p, m->S, N, NP, uniform_mix, m->tab.p, d_gp.p);
      HIPCHK(hipGetLastError());
      if (gauss_params)
        HIPCHK(hipMemcpy(gauss_params, d_gp.p, (size_t)n_gauss * N * 2 * sizeof(double), hipMemcpyDeviceToHost));
      else
        HIPCHK(hipDeviceSynchronize());
    }
  }
  // the user constraints, in the reference's order (hmm.py:608-614: transitions, emissions, start), whatever the
  // update flags say; transMatEpsilons alone belongs to the transition update (k_mstep_trans)
  if (m->c_trans || m->c_start)
    hipLaunchKernelGGL(k_constrain_trans, dim3(1), dim3(128), 0, 0, N, NP, (const uint8_t *)m->c_tmask.p,
                       (const double *)m->c_tval.p, (const uint8_t *)m->c_smask.p, (const double *)m->c_sval.p,
                       m->c_eps ? 1 : 0, m->lt.p, m->pi.p, m->c_status.p);
  if (m->c_emis)
    hipLaunchKernelGGL(k_constrain_emis, dim3(grid_for((int64_t)m->K * N, 64)), dim3(64), 0, 0, tr, N, NP, m->S,
                       (const uint8_t *)m->c_emask.p, (const double *)m->c_eval.p, m->tab.p, m->c_status.p);
  if (int rc = mstep_rebuild(m, tr, update_emission || m->c_emis, update_trans || m->c_trans)) return rc;
  HIPCHK(hipGetLastError());
  if (forced) {
    // the status word comes with the synchronisation every M-step ends in
    int status = 0;
    HIPCHK(hipMemcpy(&status, m->c_status.p, sizeof(int), hipMemcpyDeviceToHost));
    if (status != 0) {
      HIPCHK(hipMemcpy(m->lt.p, m->c_save.p, (size_t)NP * NP * sizeof(double), hipMemcpyDeviceToDevice));
      HIPCHK(hipMemcpy(m->pi.p, m->c_save.p + (size_t)NP * NP, (size_t)NP * sizeof(double), hipMemcpyDeviceToDevice));
      HIPCHK(hipMemcpy(m->tab.p, m->c_save.p + (size_t)NP * NP + NP, n_tab * sizeof(double), hipMemcpyDeviceToDevice));
      if (int rc = mstep_rebuild(m, tr, true, true)) return rc;
      HIPCHK(hipDeviceSynchronize());
      ++m->version;
      return fail(TEHMM_ERR_ARG, std::string("tehmm_model_mstep: ") +
                  ((status & TEHMM_CSTAT_EMIS_ZERO) ? "a forced emission row totals zero and nothing learned is left to "
                                                      "scale (the reference asserts curTotal > 0)"
                                                    : "a constrained value is not finite") +
                  "; the parameters are those from before the call");
    }
  } else {
    HIPCHK(hipDeviceSynchronize());
  }
  ++m->version;
  return TEHMM_OK;
}

// tehmm_model_set_constraints: the tables are checked, uploaded once and kept on the handle
int tehmm_model_set_constraints(tehmm_model_t *m, const uint8_t *trans_mask, const double *trans_val,
                                const uint8_t *start_mask, const double *start_val, const uint8_t *emis_mask,
                                const double *emis_val, int trans_epsilons) {
  if (!m || (trans_mask == nullptr) != (trans_val == nullptr) || (start_mask == nullptr) != (start_val == nullptr) ||
      (emis_mask == nullptr) != (emis_val == nullptr))
    return fail(TEHMM_ERR_ARG, "tehmm_model_set_constraints: NULL handle or a mask without its values");
  if (m->N > 128)
    return fail(TEHMM_ERR_UNSUPPORTED, "tehmm_model_set_constraints: N > 128 (no device-resident M-step)");
  const int N = m->N, NP = m->NP, K = m->K, S = m->S;
  // what the forced values alone decide (hmm.py:410-413, 471-472; emission.py:391-399, 410-419)
  if (trans_mask)
    for (int i = 0; i < N; ++i) {
      double tgt = 1.0;
      for (int j = 0; j < N; ++j)
        if (trans_mask[(size_t)i * N + j]) tgt -= trans_val[(size_t)i * N + j];
      if (!(tgt >= -TEHMM_DBL_EPS))
        return fail(TEHMM_ERR_ARG, "tehmm_model_set_constraints: forced transitions of state " + std::to_string(i) +
                                       " exceed 1 (or are not numbers)");
    }
  if (start_mask) {
    double tgt = 1.0;
    for (int i = 0; i < N; ++i)
      if (start_mask[i]) tgt -= start_val[i];
    if (!(tgt >= 0.0)) return fail(TEHMM_ERR_ARG, "tehmm_model_set_constraints: forced start probabilities exceed 1");
  }
  if (emis_mask)
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < N; ++j) {
        const uint8_t *mk = emis_mask + ((size_t)k * N + j) * S;
        const double *vl = emis_val + ((size_t)k * N + j) * S;
        if (m->rowcnt[k] < 2 || (mk[1] & 2)) continue;
        double tgt = 1.0;
        int forced = 0;
        for (int s = 1; s < m->rowcnt[k]; ++s)
          if (mk[s] & 1) { tgt -= vl[s]; ++forced; }
        if (!(tgt >= 0.0))
          return fail(TEHMM_ERR_ARG, "tehmm_model_set_constraints: forced emissions of track " + std::to_string(k) +
                                         ", state " + std::to_string(j) + " exceed 1 (or are not numbers)");
        if (forced == m->rowcnt[k] - 1 && tgt < 1.0)
          return fail(TEHMM_ERR_ARG, "tehmm_model_set_constraints: every symbol of track " + std::to_string(k) +
                                         ", state " + std::to_string(j) + " is forced: no symbol left for the leftover");
      }
  m->c_trans = m->c_start = m->c_emis = m->c_eps = false;
  m->c_tmask.release(); m->c_tval.release();
  m->c_smask.release(); m->c_sval.release();
  m->c_emask.release(); m->c_eval.release();
  if (!trans_mask && !start_mask && !emis_mask && !trans_epsilons) {
    m->c_save.release();
    m->c_status.release();
    return TEHMM_OK;
  }
  if (trans_mask) {
    HIPCHK(m->c_tmask.upload(trans_mask, (size_t)N * N));
    HIPCHK(m->c_tval.upload(trans_val, (size_t)N * N));
  }
  if (start_mask) {
    HIPCHK(m->c_smask.upload(start_mask, (size_t)N));
    HIPCHK(m->c_sval.upload(start_val, (size_t)N));
  }
  if (emis_mask) {
    HIPCHK(m->c_emask.upload(emis_mask, (size_t)K * N * S));
    HIPCHK(m->c_eval.upload(emis_val, (size_t)K * N * S));
  }
  HIPCHK(m->c_save.alloc((size_t)NP * NP + NP + (size_t)(m->R + 1) * NP));
  HIPCHK(m->c_status.alloc(1));
  m->c_trans = trans_mask != nullptr;
  m->c_start = start_mask != nullptr;
  m->c_emis = emis_mask != nullptr;
  m->c_eps = trans_epsilons != 0;
  return TEHMM_OK;
}

int tehmm_model_get_params(tehmm_model_t *m, double *log_transmat, double *log_startprob, double *logProbs) {
  if (!m) return fail(TEHMM_ERR_ARG, "tehmm_model_get_params: NULL handle");
  const int N = m->N, NP = m->NP, K = m->K, S = m->S;
  if (log_transmat) {
    std::vector<double> h((size_t)NP * NP);
    HIPCHK(hipMemcpy(h.data(), m->lt.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) log_transmat[(size_t)i * N + j] = h[(size_t)i * NP + j];
  }
  if (log_startprob) {
    std::vector<double> h((size_t)NP);
    HIPCHK(hipMemcpy(h.data(), m->pi.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i) log_startprob[i] = h[(size_t)i];
  }
  if (logProbs) {
    // only the cells the packed table holds are written (symbols 0 .. numSymbols of each track); the
    // caller's padding cells keep their values
    std::vector<double> h((size_t)(m->R + 1) * NP);
    HIPCHK(hipMemcpy(h.data(), m->tab.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
      for (int s = 0; s < m->rowcnt[k]; ++s)
        for (int j = 0; j < N; ++j)
          logProbs[((size_t)k * N + j) * S + s] = h[(size_t)(m->rowbase[k] + s) * NP + j];
  }
  return TEHMM_OK;
}
