// tehmm_scaling_host.inc -- host side of the kernels in tehmm_scaling.hip.h (included by tehmm_hip.hip, behind
// tehmm_trackio_host.inc whose TrkIndex and timing list it uses): rows won per record, and the float paint.

int tehmm_track_rows_won(int64_t T, int K, const int64_t *rec_offsets, const int64_t *rec_start,
                         const int64_t *rec_end, int64_t *won, int64_t *uncovered) {
  const std::string who = "tehmm_track_rows_won";
  t_trackio_timing.clear();
  if (int rc = trk_check_lists(who, T, K, rec_offsets, rec_start, rec_end)) return rc;
  const int64_t n_rec = rec_offsets[K];
  if (!uncovered || (n_rec > 0 && !won)) return fail(TEHMM_ERR_ARG, who + ": NULL output");
  if (T == 0) {
    std::fill(uncovered, uncovered + K, (int64_t)0);
    std::fill(won, won + n_rec, (int64_t)0);
    return TEHMM_OK;
  }
  TrkIndex ix;
  ix.plan(K, rec_offsets);
  SegClock clk;
  DBuf<unsigned long long> d_cnt;      // [n_rec] rows won, then [K] uncovered rows
  HIPCHK(clk.mark("start"));
  if (int rc = ix.upload(rec_start, rec_end)) return rc;
  HIPCHK(clk.mark("upload"));
  if (int rc = ix.build(who, T, K, clk)) return rc;

  HIPCHK(d_cnt.alloc((size_t)n_rec + (size_t)K));
  HIPCHK(hipMemsetAsync(d_cnt.p, 0, ((size_t)n_rec + (size_t)K) * sizeof(unsigned long long), 0));
  // a workgroup sums the uncovered rows and the whole-tile winners of its tiles in LDS: few enough workgroups that each
  // walks several tiles, enough of them that the last round of workgroups on the device is a small part of the run
  hipLaunchKernelGGL(k_trk_rows_won, dim3(grid_for(ix.n_tiles, 1, 1 << 16)), dim3(256), 0, 0, ix.tracks(T, K), ix.lv,
                     ix.n_tiles, d_cnt.p, d_cnt.p + n_rec);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("count"));
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counters are copied out as they are");
  HIPCHK(hipMemcpy(won, d_cnt.p, (size_t)n_rec * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(uncovered, d_cnt.p + n_rec, (size_t)K * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_trackio_timing));
  return TEHMM_OK;
}

int tehmm_load_tracks_f32(int64_t T, int K, const float *fill, const int64_t *rec_offsets, const int64_t *rec_start,
                          const int64_t *rec_end, const float *rec_val, float *out) {
  const std::string who = "tehmm_load_tracks_f32";
  t_trackio_timing.clear();
  if (int rc = trk_check_lists(who, T, K, rec_offsets, rec_start, rec_end)) return rc;
  const int64_t n_rec = rec_offsets[K];
  if (!fill || (n_rec > 0 && !rec_val)) return fail(TEHMM_ERR_ARG, who + ": NULL argument");
  if (T > 0 && !out) return fail(TEHMM_ERR_ARG, who + ": NULL out");
  if (T == 0) return TEHMM_OK;
  TrkIndex ix;
  ix.plan(K, rec_offsets);
  SegClock clk;
  DBuf<float> d_fill, d_val, d_out;
  HIPCHK(clk.mark("start"));
  HIPCHK(d_fill.upload(fill, (size_t)K));
  if (int rc = ix.upload(rec_start, rec_end)) return rc;
  HIPCHK(d_val.upload(rec_val, (size_t)n_rec));
  HIPCHK(clk.mark("upload"));
  if (int rc = ix.build(who, T, K, clk)) return rc;

  HIPCHK(d_out.alloc((size_t)T * (size_t)K));
  hipLaunchKernelGGL(k_trk_paint_f32, dim3(grid_for(ix.n_tiles, 1, 1 << 20)), dim3(256), 0, 0, ix.tracks(T, K), ix.lv,
                     ix.n_tiles, (const float *)d_fill.p, (const float *)d_val.p, d_out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("paint"));
  HIPCHK(hipMemcpy(out, d_out.p, (size_t)T * (size_t)K * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_trackio_timing));
  return TEHMM_OK;
}
