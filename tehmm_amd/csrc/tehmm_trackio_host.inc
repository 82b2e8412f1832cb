// tehmm_trackio_host.inc -- host side of the kernels in tehmm_trackio.hip.h (included by tehmm_hip.hip, behind
// tehmm_segment_host.inc whose SegClock it uses): BED records and FASTA bases painted into a uint8 [T, K] table.

namespace {

thread_local std::vector<std::pair<const char *, double>> t_trackio_timing;      // device passes of the last call

// The record lists of a call on the device, with what the winner search of tehmm_trackio.hip.h reads: block maxima and
// running maxima of rec_end, and the tile index.  Shared by every call that walks records (tehmm_load_tracks_u8,
// tehmm_track_rows_won, tehmm_load_tracks_f32).
struct TrkIndex {
  std::vector<std::vector<int64_t>> base;      // [level][K + 1]; [0] = rec_offsets
  int64_t n_rec = 0, tree_total = 0, n_tiles = 0;
  int n_levels = 0;
  DBuf<int64_t> d_base, d_start, d_end, d_tree, d_run0, d_trun;
  DBuf<int32_t> d_tidx;
  DBuf<unsigned long long> d_viol;
  TrkLevels lv;

  // entries of every level per track: level l + 1 has one entry per 64 of level l, and levels are added until the top
  // one is a single entry in every track (the first pass is also the one that checks the records)
  void plan(int K, const int64_t *rec_offsets) {
    base.assign(1, std::vector<int64_t>(rec_offsets, rec_offsets + K + 1));
    n_rec = rec_offsets[K];
    tree_total = 0;
    if (n_rec > 0)
      for (;;) {
        const std::vector<int64_t> &below = base.back();
        std::vector<int64_t> b((size_t)K + 1);
        int64_t widest = 0;
        b[0] = tree_total;
        for (int k = 0; k < K; ++k) {
          const int64_t cnt = (below[(size_t)k + 1] - below[(size_t)k] + TEHMM_TRACKIO_FAN - 1) / TEHMM_TRACKIO_FAN;
          b[(size_t)k + 1] = b[(size_t)k] + cnt;
          widest = std::max(widest, cnt);
        }
        tree_total = b[(size_t)K];
        base.push_back(b);
        if (widest <= 1 || (int)base.size() > TEHMM_TRACKIO_MAX_LEVELS) break;
      }
    n_levels = (int)base.size() - 1;
  }

  int upload(const int64_t *rec_start, const int64_t *rec_end) {
    std::vector<int64_t> flat;
    for (auto &b : base) flat.insert(flat.end(), b.begin(), b.end());
    HIPCHK(d_base.upload(flat.data(), flat.size()));
    HIPCHK(d_start.upload(rec_start, (size_t)n_rec));
    HIPCHK(d_end.upload(rec_end, (size_t)n_rec));
    return TEHMM_OK;
  }

  // the levels (with the record check) and the tile index; marks "tree" on clk either way
  int build(const std::string &who, int64_t T, int K, SegClock &clk) {
    lv.n = n_levels;
    for (int l = 0; l <= TEHMM_TRACKIO_MAX_LEVELS; ++l) {
      lv.ptr[l] = lv.run[l] = nullptr;
      lv.base[l] = d_base.p;
    }
    if (n_rec > 0) {
      HIPCHK(d_tree.alloc((size_t)tree_total));
      HIPCHK(d_trun.alloc((size_t)tree_total));
      HIPCHK(d_run0.alloc((size_t)n_rec));
      HIPCHK(d_viol.alloc(1));
      HIPCHK(hipMemsetAsync(d_viol.p, 0xff, sizeof(unsigned long long), 0));
      lv.ptr[0] = d_end.p;
      lv.run[0] = d_run0.p;
      for (int l = 1; l <= n_levels; ++l) {
        lv.ptr[l] = d_tree.p;
        lv.run[l] = d_trun.p;
        lv.base[l] = d_base.p + (size_t)l * ((size_t)K + 1);
        const int64_t n_out = base[(size_t)l][(size_t)K] - base[(size_t)l][0];
        const dim3 grid(grid_for(n_out, 4, 1 << 16)), block(256);
        if (l == 1)
          hipLaunchKernelGGL((k_trk_level<true>), grid, block, 0, 0, K, T, lv.ptr[0], lv.base[0],
                             (const int64_t *)d_start.p, d_run0.p, d_tree.p, lv.base[1], d_viol.p);
        else
          hipLaunchKernelGGL((k_trk_level<false>), grid, block, 0, 0, K, T, lv.ptr[l - 1], lv.base[l - 1],
                             (const int64_t *)nullptr, d_trun.p, d_tree.p, lv.base[l], (unsigned long long *)nullptr);
      }
      HIPCHK(hipGetLastError());
      unsigned long long viol = 0;
      HIPCHK(hipMemcpy(&viol, d_viol.p, sizeof(viol), hipMemcpyDeviceToHost));
      if (viol != ~0ull) {
        HIPCHK(clk.mark("tree"));
        return fail(TEHMM_ERR_ARG, who + ": record " + std::to_string(viol) +
                                       " starts before its predecessor in the track, or fails 0 <= start < end <= T");
      }
    }
    n_tiles = (T + TEHMM_TRACKIO_TILE - 1) / TEHMM_TRACKIO_TILE;
    HIPCHK(d_tidx.alloc((size_t)(n_tiles + 1) * (size_t)K));
    hipLaunchKernelGGL(k_trk_tile_index, dim3(grid_for((n_tiles + 1) * K, 256, 1 << 20)), dim3(256), 0, 0, K, n_tiles,
                       (const int64_t *)d_base.p, (const int64_t *)d_start.p, d_tidx.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("tree"));
    return TEHMM_OK;
  }

  TrkTracks tracks(int64_t T, int K) const {
    TrkTracks tr = {};
    tr.T = T;
    tr.K = K;
    tr.rec_base = d_base.p;
    tr.start = d_start.p;
    tr.end = d_end.p;
    tr.tile_index = d_tidx.p;
    return tr;
  }
};

// what every call checks of T, K and its record lists before any device call
int trk_check_lists(const std::string &who, int64_t T, int K, const int64_t *rec_offsets, const int64_t *rec_start,
                    const int64_t *rec_end) {
  if (T < 0) return fail(TEHMM_ERR_ARG, who + ": T < 0");
  if (K < 1 || K > TEHMM_TRACKIO_MAX_TRACKS) return fail(TEHMM_ERR_ARG, who + ": K outside 1..128");
  if (!rec_offsets) return fail(TEHMM_ERR_ARG, who + ": NULL argument");
  if (rec_offsets[0] != 0) return fail(TEHMM_ERR_ARG, who + ": offsets start at 0");
  for (int k = 0; k < K; ++k)
    if (rec_offsets[k + 1] < rec_offsets[k])
      return fail(TEHMM_ERR_ARG, who + ": rec_offsets decrease at track " + std::to_string(k));
  if (rec_offsets[K] > 0 && (!rec_start || !rec_end)) return fail(TEHMM_ERR_ARG, who + ": NULL record column");
  if (rec_offsets[K] > 0x7fffffffll) return fail(TEHMM_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 records");
  return TEHMM_OK;
}

}  // namespace

int64_t tehmm_trackio_tile_rows(void) { return TEHMM_TRACKIO_TILE; }

int tehmm_trackio_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds)
    return fail(TEHMM_ERR_ARG, "tehmm_trackio_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_trackio_timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_load_tracks_u8(int64_t T, int K, const uint8_t *fill, const uint8_t *kind, const int64_t *rec_offsets,
                         const int64_t *rec_start, const int64_t *rec_end, const uint8_t *rec_sym0,
                         const uint8_t *rec_sym, const int64_t *seq_offsets, const uint8_t *seq_bytes,
                         const uint8_t *seq_lut, uint8_t *data) {
  const std::string who = "tehmm_load_tracks_u8";
  t_trackio_timing.clear();
  if (int rc = trk_check_lists(who, T, K, rec_offsets, rec_start, rec_end)) return rc;
  if (!fill || !kind || !seq_offsets) return fail(TEHMM_ERR_ARG, who + ": NULL argument");
  if (T > 0 && !data) return fail(TEHMM_ERR_ARG, who + ": NULL data");
  if (seq_offsets[0] != 0) return fail(TEHMM_ERR_ARG, who + ": offsets start at 0");
  int n_seq = 0;
  std::vector<int32_t> seq_rank((size_t)K, 0);
  for (int k = 0; k < K; ++k) {
    if (kind[k] > 1) return fail(TEHMM_ERR_ARG, who + ": kind of track " + std::to_string(k) + " is neither 0 nor 1");
    if (seq_offsets[k + 1] < seq_offsets[k])
      return fail(TEHMM_ERR_ARG, who + ": seq_offsets decrease at track " + std::to_string(k));
    if (kind[k] && rec_offsets[k + 1] != rec_offsets[k])
      return fail(TEHMM_ERR_ARG, who + ": sequence track " + std::to_string(k) + " has records");
    if (seq_offsets[k + 1] - seq_offsets[k] != (kind[k] ? T : 0))
      return fail(TEHMM_ERR_ARG, who + ": track " + std::to_string(k) +
                                     " must own T sequence bytes if it is a sequence track and none otherwise");
    seq_rank[(size_t)k] = n_seq;
    n_seq += kind[k];
  }
  const int64_t n_rec = rec_offsets[K];
  if (n_rec > 0 && (!rec_sym0 || !rec_sym)) return fail(TEHMM_ERR_ARG, who + ": NULL record column");
  if (n_seq > 0 && T > 0 && (!seq_bytes || !seq_lut)) return fail(TEHMM_ERR_ARG, who + ": NULL sequence bytes or lut");
  if (T == 0) return TEHMM_OK;

  TrkIndex ix;
  ix.plan(K, rec_offsets);
  SegClock clk;
  DBuf<uint8_t> d_fill, d_kind, d_sym0, d_sym, d_seq, d_lut, d_data;
  DBuf<int32_t> d_rank;
  HIPCHK(clk.mark("start"));
  HIPCHK(d_fill.upload(fill, (size_t)K));
  HIPCHK(d_kind.upload(kind, (size_t)K));
  HIPCHK(d_rank.upload(seq_rank.data(), (size_t)K));
  if (int rc = ix.upload(rec_start, rec_end)) return rc;
  HIPCHK(d_sym0.upload(rec_sym0, (size_t)n_rec));
  HIPCHK(d_sym.upload(rec_sym, (size_t)n_rec));
  const int64_t stride = (T + 7) / 8 * 8;
  if (n_seq > 0) {
    HIPCHK(d_seq.alloc((size_t)(stride * n_seq)));
    HIPCHK(d_lut.upload(seq_lut, (size_t)n_seq * 256));
    for (int q = 0; q < n_seq; ++q) {      // the pad behind the last base of a track reads as "no base"
      HIPCHK(hipMemsetAsync(d_seq.p + (size_t)(stride * q + stride - 8), 0, 8, 0));
      HIPCHK(hipMemcpy(d_seq.p + (size_t)(stride * q), seq_bytes + (size_t)(T * q), (size_t)T, hipMemcpyHostToDevice));
    }
  }
  HIPCHK(clk.mark("upload"));

  if (int rc = ix.build(who, T, K, clk)) return rc;

  HIPCHK(d_data.alloc((size_t)T * (size_t)K));
  TrkTracks tr = ix.tracks(T, K);
  tr.fill = d_fill.p;
  tr.kind = d_kind.p;
  tr.sym0 = d_sym0.p;
  tr.sym = d_sym.p;
  tr.seq = d_seq.p;
  tr.seq_stride = stride;
  tr.seq_rank = d_rank.p;
  tr.lut = d_lut.p;
  hipLaunchKernelGGL(k_trk_paint, dim3(grid_for(ix.n_tiles, 1, 1 << 20)), dim3(256), (size_t)TEHMM_TRACKIO_TILE * K, 0,
                     tr, ix.lv, ix.n_tiles, d_data.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("paint"));
  HIPCHK(hipMemcpy(data, d_data.p, (size_t)T * (size_t)K, hipMemcpyDeviceToHost));
  HIPCHK(clk.mark("download"));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(clk.finish(t_trackio_timing));
  return TEHMM_OK;
}
