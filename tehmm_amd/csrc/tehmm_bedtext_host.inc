// tehmm_bedtext_host.inc -- host side of the kernels in tehmm_bedtext.hip.h (included by tehmm_hip.hip, behind
// tehmm_segment_host.inc whose SegClock it uses): the per-row BED text of teHmmEval formatted on the device, in
// stripes whose copy-back overlaps the fwrite of the stripe before (DESIGN.md section 5s).

namespace {

struct BtCounters {
  int64_t rows = 0, bytes = 0, host_rows = 0;
  std::vector<std::pair<const char *, double>> timing;      // device passes and host waits of the last call, milliseconds
};
thread_local BtCounters t_bt;

constexpr int64_t kBtStripeDefault = (int64_t)4 << 20, kBtStripeMax = (int64_t)1 << 28;

// 10^k = (hi + lo)(1 + d), |d| < 2^-105: hi holds the top 53 bits of 10^k (k >= 0: exact integer arithmetic) or of
// floor(2^s / 10^-k) with more than 170 significant bits (k < 0), lo the 64 bits behind them rounded to a double
void bt_pow10_dd(int k, double *hi, double *lo) {
  std::vector<uint32_t> a(1, 1u);                // little endian; the value is a 2^-sh
  int sh = 0;
  if (k >= 0) {
    for (int i = 0; i < k; ++i) {
      uint64_t c = 0;
      for (auto &w : a) {
        c += (uint64_t)w * 10u;
        w = (uint32_t)c;
        c >>= 32;
      }
      if (c) a.push_back((uint32_t)c);
    }
  } else {
    const int n = -k;
    sh = n * 10 / 3 + 200;                       // > n log2(10) + 170
    a.assign((size_t)sh / 32 + 1, 0u);
    a[(size_t)sh / 32] = 1u << (sh % 32);
    for (int i = 0; i < n; ++i) {                // (floor of a floor is the floor of the whole quotient)
      uint64_t r = 0;
      for (size_t j = a.size(); j-- > 0;) {
        r = (r << 32) | a[j];
        a[j] = (uint32_t)(r / 10u);
        r %= 10u;
      }
      while (a.size() > 1 && a.back() == 0) a.pop_back();
    }
  }
  int L = (int)a.size() * 32;                    // bit length
  while (L > 0 && !((a[(size_t)(L - 1) / 32] >> ((L - 1) % 32)) & 1u)) --L;
  auto bits = [&](int top, int cnt) {            // bits top, top - 1, ... (cnt of them); below bit 0: zeros
    uint64_t v = 0;
    for (int b = top; b > top - cnt; --b) {
      v <<= 1;
      if (b >= 0 && ((a[(size_t)b / 32] >> (b % 32)) & 1u)) v |= 1u;
    }
    return v;
  };
  *hi = std::ldexp((double)bits(L - 1, 53), L - 53 - sh);
  *lo = std::ldexp((double)bits(L - 54, 64), L - 53 - 64 - sh);
}

const std::vector<BtDD> &bt_pow10_table() {
  static const std::vector<BtDD> tab = [] {
    std::vector<BtDD> t((size_t)(TEHMM_BT_P10_MAX - TEHMM_BT_P10_MIN + 1));
    for (int k = TEHMM_BT_P10_MIN; k <= TEHMM_BT_P10_MAX; ++k) bt_pow10_dd(k, &t[(size_t)(k - TEHMM_BT_P10_MIN)].hi, &t[(size_t)(k - TEHMM_BT_P10_MIN)].lo);
    return t;
  }();
  return tab;
}

// tehmm_write_bed's text of a value, in the record layout of tehmm_bedtext.hip.h
void bt_host_record(double v, uint8_t *rec) {
  char num[64];
  int k = std::snprintf(num, sizeof(num), "%.12g", v);
  bool plain = true;
  for (int q = 0; q < k; ++q) plain = plain && ((num[q] >= '0' && num[q] <= '9') || num[q] == '-');
  if (plain) {
    num[k++] = '.';
    num[k++] = '0';
  }
  if (k > TEHMM_BT_REC - 1) k = TEHMM_BT_REC - 1;      // (%.12g of a double is at most 19 characters)
  std::memset(rec, 0, TEHMM_BT_REC);
  for (int q = 0; q < k; ++q) rec[k - 1 - q] = (uint8_t)num[q];
  rec[TEHMM_BT_REC - 1] = (uint8_t)k;
}

struct BtStream {
  hipStream_t s = nullptr;
  hipEvent_t emitted[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
  void *pin[2] = {nullptr, nullptr};
  size_t pin_bytes[2] = {0, 0};
  FILE *f = nullptr;
  ~BtStream() {
    if (s) (void)hipStreamSynchronize(s);
    for (int i = 0; i < 2; ++i) {
      if (emitted[i]) (void)hipEventDestroy(emitted[i]);
      if (copied[i]) (void)hipEventDestroy(copied[i]);
      if (pin[i]) (void)tehmm_host_free(pin[i]);
    }
    if (s) (void)hipStreamDestroy(s);
    if (f) std::fclose(f);
  }
};

// The tables of one call.  Columns are device pointers indexed by row (row 0 = the first row of table 0).
struct BtCall {
  const char *who;
  const char *path;
  int append;
  int n_tables;
  const char *const *chroms;
  const int64_t *table_start, *table_end, *row_offsets;
  const int64_t *const *segOffsets;
  const int32_t *const *maskOffsets;
  const int64_t *n_mask;
  const char *const *headers;
  int kind;
  const int64_t *d_states;
  const double *d_values;
  int n_names;
  const char *const *names;
  int shift;
  int64_t stripe_rows;
};

int bt_check_args(const BtCall &c) {
  const std::string who = c.who;
  if (!c.path || c.n_tables < 0 || (c.n_tables > 0 && (!c.chroms || !c.table_start || !c.table_end || !c.row_offsets)))
    return fail(TEHMM_ERR_ARG, who + ": bad argument");
  if (c.kind != TEHMM_BED_NAMES && c.kind != TEHMM_BED_INT && c.kind != TEHMM_BED_VALUE)
    return fail(TEHMM_ERR_ARG, who + ": unknown kind of column 4");
  if (c.kind == TEHMM_BED_NAMES && (c.n_names < 0 || c.n_names > TEHMM_LARGE_MAX || (c.n_names > 0 && !c.names)))
    return fail(TEHMM_ERR_ARG, who + ": names needs 0 to 1024 names");
  if (c.stripe_rows < 0 || c.stripe_rows > kBtStripeMax) return fail(TEHMM_ERR_ARG, who + ": bad stripe_rows");
  if (c.maskOffsets && !c.n_mask) return fail(TEHMM_ERR_ARG, who + ": maskOffsets without n_mask");
  if (c.n_tables > 0 && c.row_offsets[0] != 0) return fail(TEHMM_ERR_ARG, who + ": row_offsets must start at 0");
  for (int t = 0; t < c.n_tables; ++t) {
    if (!c.chroms[t]) return fail(TEHMM_ERR_ARG, who + ": NULL chrom");
    const int64_t n = c.row_offsets[t + 1] - c.row_offsets[t];
    if (n < 0) return fail(TEHMM_ERR_ARG, who + ": row_offsets must not descend");
    if (c.maskOffsets && c.maskOffsets[t] && n > 0) {
      const int64_t *so = c.segOffsets ? c.segOffsets[t] : nullptr;
      const int64_t dmax = so ? so[n - 1] - so[0] : n - 1;
      if (c.n_mask[t] <= 0 || dmax >= c.n_mask[t])
        return fail(TEHMM_ERR_ARG, who + ": maskOffsets shorter than the table");
      // (the offsets index the mask block on the device: every one of them has to lie inside it)
      for (int64_t i = 1; so && i < n; ++i)
        if (so[i] < so[i - 1]) return fail(TEHMM_ERR_ARG, who + ": segOffsets descend in a masked table");
    }
  }
  return TEHMM_OK;
}

int bt_write(const BtCall &c) {
  const std::string who = c.who;
  t_bt = BtCounters();
  const auto wall0 = std::chrono::steady_clock::now();
  const int T = c.n_tables;
  const int64_t rows = T > 0 ? c.row_offsets[T] : 0;
  const int64_t items = rows + T;
  // ---- tables, blob, joined offset arrays -------------------------------------------------------------------------
  std::vector<BtTable> tab((size_t)T);
  std::vector<uint8_t> blob;
  std::vector<int64_t> seg;
  std::vector<int32_t> mask;
  for (int t = 0; t < T; ++t) {
    BtTable &b = tab[(size_t)t];
    b.row0 = c.row_offsets[t];
    b.row1 = c.row_offsets[t + 1];
    b.key = b.row0 + t;
    b.start = c.table_start[t];
    b.end = c.table_end[t];
    const int64_t n = b.row1 - b.row0;
    b.seg0 = b.mask0 = -1;
    if (n > 0 && c.segOffsets && c.segOffsets[t]) {
      b.seg0 = (int64_t)seg.size();
      seg.insert(seg.end(), c.segOffsets[t], c.segOffsets[t] + n);
    }
    if (n > 0 && c.maskOffsets && c.maskOffsets[t]) {
      b.mask0 = (int64_t)mask.size();
      mask.insert(mask.end(), c.maskOffsets[t], c.maskOffsets[t] + c.n_mask[t]);
    }
    const size_t cl = std::strlen(c.chroms[t]), hl = c.headers && c.headers[t] ? std::strlen(c.headers[t]) : 0;
    if (blob.size() + cl + hl > 0x7fffffffu) return fail(TEHMM_ERR_UNSUPPORTED, who + ": chroms and headers beyond 2 GB");
    b.chrom_off = (int32_t)blob.size();
    b.chrom_len = (int32_t)cl;
    blob.insert(blob.end(), c.chroms[t], c.chroms[t] + cl);
    b.hdr_off = (int32_t)blob.size();
    b.hdr_len = (int32_t)hl;
    if (hl) blob.insert(blob.end(), c.headers[t], c.headers[t] + hl);
  }
  std::vector<uint8_t> nblob;
  std::vector<int32_t> noff;
  if (c.kind == TEHMM_BED_NAMES) {
    noff.push_back(0);
    for (int s = 0; s < c.n_names; ++s) {
      if (!c.names[s]) return fail(TEHMM_ERR_ARG, who + ": NULL name");
      const size_t l = std::strlen(c.names[s]);
      if (nblob.size() + l > 0x7fffffffu) return fail(TEHMM_ERR_UNSUPPORTED, who + ": names beyond 2 GB");
      nblob.insert(nblob.end(), c.names[s], c.names[s] + l);
      noff.push_back((int32_t)nblob.size());
    }
  }
  DBuf<BtTable> d_tab;
  DBuf<uint8_t> d_blob, d_nblob;
  DBuf<int64_t> d_seg;
  DBuf<int32_t> d_mask, d_noff;
  DBuf<BtDD> d_pow;
  DBuf<unsigned long long> d_ctr;              // [0] the stripe's bytes (the scan's total), [1] flagged rows, [2] violation
  unsigned long long ctr[3] = {0, 0, ~0ull};
  HIPCHK(d_ctr.upload(ctr, 3));
  // ---- every state has a name, before the file is touched ---------------------------------------------------------
  if (c.kind == TEHMM_BED_NAMES && rows > 0) {
    hipLaunchKernelGGL(k_bt_check_states, dim3(grid_for(rows, 256, 1 << 14)), dim3(256), 0, 0, rows, c.d_states,
                       c.n_names, d_ctr.p + 2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
    if (ctr[2] != ~0ull)
      return fail(TEHMM_ERR_ARG, who + ": state without a name in row " + std::to_string(ctr[2]));
  }
  BtStream io;
  io.f = std::fopen(c.path, c.append ? "a" : "w");
  if (!io.f) return fail(TEHMM_ERR_ARG, who + ": cannot open " + c.path);
  if (items == 0) {
    FILE *f = io.f;
    io.f = nullptr;
    if (std::fclose(f) != 0) return fail(TEHMM_ERR_ARG, who + ": close failed");
    return TEHMM_OK;
  }
  HIPCHK(d_tab.upload(tab.data(), tab.size()));
  HIPCHK(d_blob.upload(blob.data(), blob.size()));
  HIPCHK(d_seg.upload(seg.data(), seg.size()));
  HIPCHK(d_mask.upload(mask.data(), mask.size()));
  HIPCHK(d_nblob.upload(nblob.data(), nblob.size()));
  HIPCHK(d_noff.upload(noff.data(), noff.size()));
  BtJob job;
  job.tab = d_tab.p;
  job.n_tables = T;
  job.seg = d_seg.p;
  job.mask = d_mask.p;
  job.blob = d_blob.p;
  job.kind = c.kind;
  job.shift = c.shift ? 1 : 0;
  job.states = c.d_states;
  job.values = c.d_values;
  job.names = d_nblob.p;
  job.name_off = d_noff.p;
  job.n_names = c.n_names;
  job.pow10 = nullptr;
  const bool vals = c.kind == TEHMM_BED_VALUE;
  if (vals) {
    const std::vector<BtDD> &pw = bt_pow10_table();
    HIPCHK(d_pow.upload(pw.data(), pw.size()));
    job.pow10 = d_pow.p;
  }
  // ---- stripes ----------------------------------------------------------------------------------------------------
  const int64_t S = std::min(items, c.stripe_rows > 0 ? c.stripe_rows : kBtStripeDefault);
  const int64_t nb_max = (S + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK;
  DBuf<uint32_t> d_count, d_fitem;
  DBuf<int64_t> d_off, d_blk;
  DBuf<uint8_t> d_rec, d_frec, d_text[2];
  DBuf<double> d_fval;
  HIPCHK(d_count.alloc((size_t)S));
  HIPCHK(d_off.alloc((size_t)S));
  HIPCHK(d_blk.alloc((size_t)nb_max));
  if (vals) {
    HIPCHK(d_rec.alloc((size_t)S * TEHMM_BT_REC));
    HIPCHK(d_fitem.alloc((size_t)S));
    HIPCHK(d_fval.alloc((size_t)S));
  }
  HIPCHK(hipStreamCreateWithFlags(&io.s, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(hipEventCreateWithFlags(&io.emitted[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&io.copied[i], hipEventDisableTiming));
  }
  SegClock clk;
  const dim3 block(256);
  int64_t *d_total = (int64_t *)d_ctr.p;
  std::vector<uint32_t> fitem;
  std::vector<double> fval;
  std::vector<uint8_t> frec;
  double ms_wait = 0.0, ms_write = 0.0;
  size_t prev_bytes = 0;
  auto scan = [&](int64_t n) {
    const unsigned nb = (unsigned)((n + TEHMM_SCAN_BLOCK - 1) / TEHMM_SCAN_BLOCK);
    hipLaunchKernelGGL(k_msk_blocksum, dim3(nb), block, 0, 0, n, (const uint32_t *)d_count.p, d_blk.p);
    hipLaunchKernelGGL(k_tsd_scan_blocks, dim3(1), block, 0, 0, (int64_t)nb, d_blk.p, d_total);
    hipLaunchKernelGGL(k_msk_offsets, dim3(nb), block, 0, 0, n, (const uint32_t *)d_count.p, (const int64_t *)d_blk.p,
                       d_off.p);
  };
  // the stripe before: wait for its copy, write it
  auto flush = [&](int slot, size_t bytes) -> int {
    auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipEventSynchronize(io.copied[slot]));
    auto t1 = std::chrono::steady_clock::now();
    if (bytes && std::fwrite(io.pin[slot], 1, bytes, io.f) != bytes) return fail(TEHMM_ERR_ARG, who + ": write failed");
    auto t2 = std::chrono::steady_clock::now();
    ms_wait += std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms_write += std::chrono::duration<double, std::milli>(t2 - t1).count();
    return TEHMM_OK;
  };
  int64_t stripe = 0;
  for (int64_t i0 = 0; i0 < items; i0 += S, ++stripe) {
    const int slot = (int)(stripe & 1);
    const int64_t n = std::min(S, items - i0);
    const dim3 grid((unsigned)((n + 255) / 256));
    HIPCHK(clk.mark("host"));
    if (vals) HIPCHK(hipMemsetAsync(d_ctr.p + 1, 0, sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_bt_measure, grid, block, 0, 0, job, i0, n, d_count.p, d_rec.p, d_ctr.p + 1, d_fitem.p, d_fval.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("measure"));
    scan(n);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("scan"));
    HIPCHK(hipMemcpy(ctr, d_ctr.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (vals && ctr[1] > 0) {                  // the rows the device did not certify: the host's snprintf
      const size_t nf = (size_t)ctr[1];
      if (nf > (size_t)n) return fail(TEHMM_ERR_HIP, who + ": inconsistent flagged count");
      fitem.resize(nf);
      fval.resize(nf);
      frec.resize(nf * TEHMM_BT_REC);
      HIPCHK(hipMemcpy(fitem.data(), d_fitem.p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(fval.data(), d_fval.p, nf * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t q = 0; q < nf; ++q) bt_host_record(fval[q], frec.data() + q * TEHMM_BT_REC);
      HIPCHK(d_frec.ensure(frec.size()));
      HIPCHK(hipMemcpy(d_frec.p, frec.data(), frec.size(), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_bt_patch, dim3((unsigned)((nf + 255) / 256)), block, 0, 0, (int64_t)nf,
                         (const uint32_t *)d_fitem.p, (const uint8_t *)d_frec.p, d_count.p, d_rec.p);
      scan(n);
      HIPCHK(hipGetLastError());
      HIPCHK(clk.mark("patch"));
      HIPCHK(hipMemcpy(ctr, d_ctr.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
      t_bt.host_rows += (int64_t)nf;
    }
    const size_t bytes = (size_t)ctr[0];
    // (the block of this slot was written out two stripes ago: nothing reads or fills it now)
    if (d_text[slot].n < bytes + 16) HIPCHK(d_text[slot].alloc(bytes + bytes / 8 + 16));
    if (io.pin_bytes[slot] < bytes) {
      if (io.pin[slot]) (void)tehmm_host_free(io.pin[slot]);
      io.pin[slot] = nullptr;
      io.pin_bytes[slot] = 0;
      const size_t want = bytes + bytes / 8 + 4096;
      int rc = tehmm_host_alloc(want, &io.pin[slot]);
      if (rc != TEHMM_OK) return rc;
      io.pin_bytes[slot] = want;
    }
    hipLaunchKernelGGL(k_bt_emit, grid, block, 0, 0, job, i0, n, (const int64_t *)d_off.p, (const int64_t *)d_total,
                       (const uint8_t *)d_rec.p, d_text[slot].p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("emit"));
    HIPCHK(hipEventRecord(io.emitted[slot], 0));
    HIPCHK(hipStreamWaitEvent(io.s, io.emitted[slot], 0));
    if (bytes) HIPCHK(hipMemcpyAsync(io.pin[slot], d_text[slot].p, bytes, hipMemcpyDeviceToHost, io.s));
    HIPCHK(hipEventRecord(io.copied[slot], io.s));
    if (stripe > 0) {
      int rc = flush(slot ^ 1, prev_bytes);
      if (rc != TEHMM_OK) return rc;
    }
    prev_bytes = bytes;
    t_bt.bytes += (int64_t)bytes;
  }
  {
    int rc = flush((int)((stripe - 1) & 1), prev_bytes);
    if (rc != TEHMM_OK) return rc;
  }
  HIPCHK(hipDeviceSynchronize());
  FILE *f = io.f;
  io.f = nullptr;
  if (std::fclose(f) != 0) return fail(TEHMM_ERR_ARG, who + ": close failed");
  t_bt.rows = rows;
  // device passes summed over the stripes, then the host's two waits and the whole call
  std::vector<std::pair<const char *, double>> marks;
  HIPCHK(clk.finish(marks));
  static const char *const order[] = {"measure", "scan", "patch", "emit", "host"};
  for (const char *name : order) {
    double sum = 0.0;
    bool any = false;
    for (auto &m : marks)
      if (std::strcmp(m.first, name) == 0) {
        sum += m.second;
        any = true;
      }
    if (any) t_bt.timing.emplace_back(name, sum);
  }
  t_bt.timing.emplace_back("copy_wait", ms_wait);
  t_bt.timing.emplace_back("fwrite", ms_write);
  t_bt.timing.emplace_back("wall", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count());
  return TEHMM_OK;
}

}  // namespace

int tehmm_bed_text_last_counters(int64_t *rows, int64_t *bytes, int64_t *host_rows) {
  if (rows) *rows = t_bt.rows;
  if (bytes) *bytes = t_bt.bytes;
  if (host_rows) *host_rows = t_bt.host_rows;
  return TEHMM_OK;
}

int tehmm_bed_text_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_bed_text_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_bt.timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_bed_text_format_value(double x, char *text, int *certified) {
  if (!text || !certified) return fail(TEHMM_ERR_ARG, "tehmm_bed_text_format_value: NULL argument");
  BtRec r;
  *certified = bt_format(x, bt_pow10_table().data(), r) ? 1 : 0;
  uint8_t rec[TEHMM_BT_REC];
  if (*certified) {
    const uint64_t w[3] = {r.t0, r.t1, r.t2};
    std::memcpy(rec, w, sizeof(rec));
    rec[TEHMM_BT_REC - 1] = (uint8_t)r.len;
  } else {
    bt_host_record(x, rec);
  }
  const int len = rec[TEHMM_BT_REC - 1];
  for (int q = 0; q < len; ++q) text[q] = (char)rec[len - 1 - q];
  text[len] = 0;
  return TEHMM_OK;
}

int tehmm_bed_text_write(const char *path, int append, int n_tables, const char *const *chroms, const int64_t *table_start,
                         const int64_t *table_end, const int64_t *row_offsets, const int64_t *const *segOffsets,
                         const int32_t *const *maskOffsets, const int64_t *n_mask, const char *const *headers, int kind,
                         const int64_t *states, const double *values, int n_names, const char *const *names, int shift,
                         int64_t stripe_rows) {
  t_bt = BtCounters();
  BtCall c = {"tehmm_bed_text_write", path, append, n_tables, chroms, table_start, table_end, row_offsets, segOffsets,
              maskOffsets, n_mask, headers, kind, nullptr, nullptr, n_names, names, shift, stripe_rows};
  int rc = bt_check_args(c);
  if (rc != TEHMM_OK) return rc;
  const int64_t rows = n_tables > 0 ? row_offsets[n_tables] : 0;
  const bool vals = kind == TEHMM_BED_VALUE;
  if (rows > 0 && (vals ? !values : !states)) return fail(TEHMM_ERR_ARG, "tehmm_bed_text_write: NULL column");
  DBuf<int64_t> d_states;
  DBuf<double> d_values;
  if (vals) HIPCHK(d_values.upload(values, (size_t)rows));
  else HIPCHK(d_states.upload(states, (size_t)rows));
  c.d_states = d_states.p;
  c.d_values = d_values.p;
  return bt_write(c);
}

int tehmm_batch_bed_text_write(tehmm_model_t *m, tehmm_batch_t *b, int source, const double *mask, int use_ratios,
                               int interval0, int n_tables, const char *const *chroms, const int64_t *table_start,
                               const int64_t *table_end, const int64_t *const *segOffsets,
                               const int32_t *const *maskOffsets, const int64_t *n_mask, const char *const *headers,
                               int n_names, const char *const *names, const char *path, int append, int64_t stripe_rows) {
  const std::string who = "tehmm_batch_bed_text_write";
  t_bt = BtCounters();
  if (!b || interval0 < 0 || n_tables < 0 || interval0 + n_tables > b->n) return fail(TEHMM_ERR_ARG, who + ": bad argument");
  if (source < TEHMM_BED_SRC_VITERBI || source > TEHMM_BED_SRC_EMISSION) return fail(TEHMM_ERR_ARG, who + ": unknown source");
  const bool vals = source == TEHMM_BED_SRC_POSTERIOR || source == TEHMM_BED_SRC_EMISSION;
  if (vals && !mask) return fail(TEHMM_ERR_ARG, who + ": the source needs a state mask");
  if (source == TEHMM_BED_SRC_EMISSION && !m) return fail(TEHMM_ERR_ARG, who + ": the emission column needs the model");
  const int64_t R0 = b->h_off[(size_t)interval0], R1 = b->h_off[(size_t)(interval0 + n_tables)];
  std::vector<int64_t> row_offsets((size_t)n_tables + 1);
  for (int t = 0; t <= n_tables; ++t) row_offsets[(size_t)t] = b->h_off[(size_t)(interval0 + t)] - R0;
  BtCall c = {"tehmm_batch_bed_text_write", path, append, n_tables, chroms, table_start, table_end, row_offsets.data(),
              segOffsets, maskOffsets, n_mask, headers, vals ? TEHMM_BED_VALUE : (names ? TEHMM_BED_NAMES : TEHMM_BED_INT),
              nullptr, nullptr, n_names, names, vals ? 1 : 0, stripe_rows};
  int rc = bt_check_args(c);
  if (rc != TEHMM_OK) return rc;
  DBuf<double> d_mask, d_col;
  const int64_t rows = R1 - R0;
  switch (source) {
    case TEHMM_BED_SRC_VITERBI:
      if (!b->paths.p) return fail(TEHMM_ERR_ARG, who + ": no Viterbi result in this batch");
      c.d_states = b->paths.p + R0;
      break;
    case TEHMM_BED_SRC_MAP:
      if (!b->map_valid) return fail(TEHMM_ERR_ARG, who + ": no maximum-posterior result in this batch");
      c.d_states = b->map_paths.p + R0;
      break;
    case TEHMM_BED_SRC_POSTERIOR:
      if (!b->post.p) return fail(TEHMM_ERR_ARG, who + ": no posterior result in this batch");
      if (rows > 0) {                           // the column of tehmm_batch_posterior_masksum, left on the device
        HIPCHK(d_mask.upload(mask, (size_t)b->N));
        HIPCHK(d_col.alloc((size_t)rows));
        if (b->N > kMaxStates)
          hipLaunchKernelGGL(k_post_masksum_large, dim3(grid_for(rows * 64, 256, 256 * 32)), dim3(256), 0, 0, rows, b->N,
                             (const double *)(b->post.p + (size_t)R0 * b->N), (const double *)d_mask.p, d_col.p);
        else
          hipLaunchKernelGGL(k_post_masksum, dim3(grid_for(rows * 64, 256, 256 * 32)), dim3(256), 0, 0, rows, b->N,
                             (const double *)(b->post.p + (size_t)R0 * b->N), (const double *)d_mask.p, d_col.p);
        HIPCHK(hipGetLastError());
      }
      c.d_values = d_col.p;
      break;
    default: {
      double *col = nullptr;
      rc = emission_dist(m, b, use_ratios, mask, true, R0, R1, nullptr, "tehmm_batch_bed_text_write", &col);
      if (rc != TEHMM_OK) return rc;
      c.d_values = col;
      break;
    }
  }
  return bt_write(c);
}
