// tehmm_bedparse_host.inc -- host side of the kernels in tehmm_bedparse.hip.h (included by tehmm_hip.hip, behind
// tehmm_masking_host.inc whose msk_scan and tehmm_segment_host.inc whose SegClock it uses): a BED file's bytes parsed
// into line, field, number and value-code columns on the device (DESIGN.md section 5u).

namespace {

struct BpCounters {
  int64_t lines = 0, records = 0, host_ints = 0, host_floats = 0, code_fallbacks = 0;
  std::vector<std::pair<const char *, double>> timing;      // passes since the last open, milliseconds
};
thread_local BpCounters t_bp;

// device bytes of a parse of n_bytes of text with n_lines lines, every line kept (the peak: text, masks, line ends,
// keep flags and record indices, the tables, then one hash column: table, slots, flags, ranks, codes, first records)
int64_t bp_workspace_bytes(int64_t n_bytes, int64_t n_lines) {
  const int64_t text = n_bytes + 16 + TEHMM_BP_PAD, masks = n_bytes / 4 + 4 + n_bytes / TEHMM_BP_TILE * 12 + 64;
  const int64_t lines = n_lines * (8 + 4 + 8);
  const int64_t tables = n_lines * (8 + 8 + 4 + 8 * TEHMM_BP_COLS + 2 * 9);
  const int64_t codes = n_lines * (4 * 16 + 8 + 4 + 8 + 8 + 8);
  return text + masks + lines + tables + codes;
}

int bp_budget(const char *who, int64_t n_bytes, int64_t n_lines) {
  size_t free_b = 0, total_b = 0;
  HIPCHK(dev_mem_info(&free_b, &total_b));
  int64_t budget = (int64_t)(free_b - free_b / 8);
  if (const char *s = std::getenv("TEHMM_BED_PARSE_MAX_WORKSPACE")) budget = std::min(budget, (int64_t)std::atoll(s));
  const int64_t need = bp_workspace_bytes(n_bytes, n_lines);
  if (need > budget)
    return fail(TEHMM_ERR_UNSUPPORTED, std::string(who) + ": text and columns need " + std::to_string(need) +
                                           " bytes of device memory, the budget is " + std::to_string(budget));
  return TEHMM_OK;
}

int bp_finish_clock(SegClock &clk) {
  std::vector<std::pair<const char *, double>> marks;
  HIPCHK(hipStreamSynchronize(0));               // (the last mark may still be in flight)
  HIPCHK(clk.finish(marks));
  for (auto &m : marks) t_bp.timing.push_back(m);
  return TEHMM_OK;
}

}  // namespace

struct tehmm_bedparse {
  int64_t n = 0, lines = 0, records = 0, high = 0;
  int hash_bits = 64;
  DBuf<uint8_t> text, istat[2];
  DBuf<int64_t> line_start, line_len, ival[2];
  DBuf<int32_t> n_fields, field_off, field_len;
  BpTable tab() {
    BpTable t;
    t.line_start = line_start.p;
    t.line_len = line_len.p;
    t.n_fields = n_fields.p;
    t.field_off = field_off.p;
    t.field_len = field_len.p;
    for (int k = 0; k < 2; ++k) {
      t.ival[k] = ival[k].p;
      t.istat[k] = istat[k].p;
    }
    return t;
  }
};

int64_t tehmm_bed_parse_tile_bytes(void) { return TEHMM_BP_TILE; }

int tehmm_bed_parse_number(const char *text, int64_t len, int kind, int64_t *ivalue, double *fvalue, int *status) {
  if ((!text && len > 0) || len < 0 || !ivalue || !fvalue || !status || (kind != TEHMM_BP_INT && kind != TEHMM_BP_FLOAT))
    return fail(TEHMM_ERR_ARG, "tehmm_bed_parse_number: bad argument");
  *ivalue = 0;
  *fvalue = 0.0;
  const bool ok = kind == TEHMM_BP_INT ? bp_parse_int((const uint8_t *)text, len, ivalue)
                                       : bp_parse_float((const uint8_t *)text, len, fvalue);
  *status = ok ? TEHMM_BP_CERTIFIED : TEHMM_BP_HOST;
  return TEHMM_OK;
}

int tehmm_bed_parse_last_counters(int64_t *lines, int64_t *records, int64_t *host_ints, int64_t *host_floats,
                                  int64_t *code_fallbacks) {
  if (lines) *lines = t_bp.lines;
  if (records) *records = t_bp.records;
  if (host_ints) *host_ints = t_bp.host_ints;
  if (host_floats) *host_floats = t_bp.host_floats;
  if (code_fallbacks) *code_fallbacks = t_bp.code_fallbacks;
  return TEHMM_OK;
}

int tehmm_bed_parse_last_timing(int max_entries, const char **names, double *milliseconds) {
  if (max_entries < 0 || !names || !milliseconds) return fail(TEHMM_ERR_ARG, "tehmm_bed_parse_last_timing: bad argument");
  int n = 0;
  for (auto &e : t_bp.timing) {
    if (n >= max_entries) break;
    names[n] = e.first;
    milliseconds[n++] = e.second;
  }
  return n;
}

int tehmm_bed_parse_close(tehmm_bedparse_t *h) {
  delete h;
  return TEHMM_OK;
}

int tehmm_bed_parse_open(const void *text, int64_t n_bytes, tehmm_bedparse_t **out) {
  const char *who = "tehmm_bed_parse_open";
  t_bp = BpCounters();
  if (!out || n_bytes < 0 || (n_bytes > 0 && !text)) return fail(TEHMM_ERR_ARG, std::string(who) + ": bad argument");
  *out = nullptr;
  const int64_t n = n_bytes, tiles = (n + TEHMM_BP_TILE - 1) / TEHMM_BP_TILE, chunks = (n + 15) / 16;
  if (tiles > INT_MAX) return fail(TEHMM_ERR_UNSUPPORTED, std::string(who) + ": too many tiles");
  std::unique_ptr<tehmm_bedparse> h(new tehmm_bedparse());
  h->n = n;
  if (const char *s = std::getenv("TEHMM_BED_PARSE_HASH_BITS")) {
    h->hash_bits = std::atoi(s);
    if (h->hash_bits < 1 || h->hash_bits > 64)
      return fail(TEHMM_ERR_ARG, std::string(who) + ": TEHMM_BED_PARSE_HASH_BITS is 1 to 64");
  }
  if (n == 0) {
    *out = h.release();
    return TEHMM_OK;
  }
  // (the line count is not known yet: a line has at least one byte)
  int rc = bp_budget(who, n, 0);
  if (rc != TEHMM_OK) return rc;
  SegClock clk;
  HIPCHK(clk.mark("start"));
  const size_t padded = (size_t)chunks * 16 + TEHMM_BP_PAD;
  HIPCHK(h->text.alloc(padded));
  HIPCHK(hipMemsetAsync(h->text.p + n, 0, padded - (size_t)n, 0));
  HIPCHK(hipMemcpyAsync(h->text.p, text, (size_t)n, hipMemcpyHostToDevice, 0));
  HIPCHK(clk.mark("upload"));
  DBuf<uint32_t> d_mask, d_count, d_keep;
  DBuf<int64_t> d_toff, d_lend, d_rec;
  DBuf<unsigned long long> d_ctr;
  unsigned long long ctr[TEHMM_BP_CTRS] = {0};
  HIPCHK(d_ctr.upload(ctr, TEHMM_BP_CTRS));
  HIPCHK(d_mask.alloc((size_t)chunks));
  HIPCHK(d_count.alloc((size_t)tiles));
  const dim3 block(256);
  hipLaunchKernelGGL(k_bp_classify, dim3((unsigned)tiles), block, 0, 0, (const uint8_t *)h->text.p, n, d_mask.p,
                     d_count.p, d_ctr.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("classify"));
  int64_t L = 0;
  rc = msk_scan(tiles, d_count.p, d_toff, &L);
  if (rc != TEHMM_OK) return rc;
  HIPCHK(clk.mark("scan_tiles"));
  HIPCHK(hipMemcpy(ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
  h->lines = L;
  h->high = (int64_t)ctr[0];
  t_bp.lines = L;
  if (h->high > 0) {                            // (decoding such a file is the locale's business: the host route)
    h->text.release();
    *out = h.release();
    return bp_finish_clock(clk);
  }
  rc = bp_budget(who, n, L);
  if (rc != TEHMM_OK) return rc;
  const unsigned lblocks = (unsigned)((L + 255) / 256);
  HIPCHK(d_lend.alloc((size_t)L));
  hipLaunchKernelGGL(k_bp_lines, dim3((unsigned)tiles), block, 0, 0, chunks, (const uint32_t *)d_mask.p,
                     (const int64_t *)d_toff.p, d_lend.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("lines"));
  HIPCHK(d_keep.alloc((size_t)L));
  hipLaunchKernelGGL(k_bp_keep, dim3(lblocks), block, 0, 0, L, (const uint8_t *)h->text.p, (const uint32_t *)d_mask.p,
                     (const int64_t *)d_lend.p, d_keep.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("keep"));
  int64_t R = 0;
  rc = msk_scan(L, d_keep.p, d_rec, &R);
  if (rc != TEHMM_OK) return rc;
  HIPCHK(clk.mark("scan_lines"));
  h->records = R;
  t_bp.records = R;
  if (R > 0) {
    HIPCHK(h->line_start.alloc((size_t)R));
    HIPCHK(h->line_len.alloc((size_t)R));
    HIPCHK(h->n_fields.alloc((size_t)R));
    HIPCHK(h->field_off.alloc((size_t)R * TEHMM_BP_COLS));
    HIPCHK(h->field_len.alloc((size_t)R * TEHMM_BP_COLS));
    for (int k = 0; k < 2; ++k) {
      HIPCHK(h->ival[k].alloc((size_t)R));
      HIPCHK(h->istat[k].alloc((size_t)R));
    }
    hipLaunchKernelGGL(k_bp_fields, dim3(lblocks), block, 0, 0, L, (const uint8_t *)h->text.p, (const int64_t *)d_lend.p,
                       (const uint32_t *)d_keep.p, (const int64_t *)d_rec.p, h->tab(), d_ctr.p);
    HIPCHK(hipGetLastError());
    HIPCHK(clk.mark("fields"));
    HIPCHK(hipMemcpy(ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
    if (ctr[1] > 0) return fail(TEHMM_ERR_UNSUPPORTED, std::string(who) + ": a record of 2^31 bytes or more");
    t_bp.host_ints += (int64_t)ctr[2];
  }
  rc = bp_finish_clock(clk);
  if (rc != TEHMM_OK) return rc;
  *out = h.release();
  return TEHMM_OK;
}

int tehmm_bed_parse_counts(tehmm_bedparse_t *h, int64_t *lines, int64_t *records, int64_t *high_bytes) {
  if (!h) return fail(TEHMM_ERR_ARG, "tehmm_bed_parse_counts: NULL handle");
  if (lines) *lines = h->lines;
  if (records) *records = h->records;
  if (high_bytes) *high_bytes = h->high;
  return TEHMM_OK;
}

int tehmm_bed_parse_get_table(tehmm_bedparse_t *h, int64_t *line_start, int64_t *line_len, int32_t *n_fields,
                              int32_t *field_off, int32_t *field_len) {
  if (!h || h->high > 0) return fail(TEHMM_ERR_ARG, "tehmm_bed_parse_get_table: no parse in this handle");
  const size_t R = (size_t)h->records;
  if (R == 0) return TEHMM_OK;
  if (!line_start || !line_len || !n_fields || !field_off || !field_len)
    return fail(TEHMM_ERR_ARG, "tehmm_bed_parse_get_table: NULL argument");
  HIPCHK(hipMemcpy(line_start, h->line_start.p, R * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(line_len, h->line_len.p, R * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(n_fields, h->n_fields.p, R * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(field_off, h->field_off.p, R * TEHMM_BP_COLS * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(field_len, h->field_len.p, R * TEHMM_BP_COLS * sizeof(int32_t), hipMemcpyDeviceToHost));
  return TEHMM_OK;
}

int tehmm_bed_parse_get_numbers(tehmm_bedparse_t *h, int col, int kind, int64_t *ivalue, double *fvalue, uint8_t *status) {
  const char *who = "tehmm_bed_parse_get_numbers";
  if (!h || h->high > 0) return fail(TEHMM_ERR_ARG, std::string(who) + ": no parse in this handle");
  if (col < 0 || col >= TEHMM_BP_COLS || (kind != TEHMM_BP_INT && kind != TEHMM_BP_FLOAT))
    return fail(TEHMM_ERR_ARG, std::string(who) + ": column 0 to 5, kind 0 or 1");
  const size_t R = (size_t)h->records;
  if (R == 0) return TEHMM_OK;
  if (!status || (kind == TEHMM_BP_INT ? !ivalue : !fvalue)) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL argument");
  if (kind == TEHMM_BP_INT && (col == 1 || col == 2)) {      // parsed with the fields
    HIPCHK(hipMemcpy(ivalue, h->ival[col - 1].p, R * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, h->istat[col - 1].p, R, hipMemcpyDeviceToHost));
    return TEHMM_OK;
  }
  DBuf<int64_t> d_i;
  DBuf<double> d_f;
  DBuf<uint8_t> d_s;
  DBuf<unsigned long long> d_ctr;
  unsigned long long ctr[TEHMM_BP_CTRS] = {0};
  HIPCHK(d_ctr.upload(ctr, TEHMM_BP_CTRS));
  if (kind == TEHMM_BP_INT) HIPCHK(d_i.alloc(R));
  else HIPCHK(d_f.alloc(R));
  HIPCHK(d_s.alloc(R));
  SegClock clk;
  HIPCHK(clk.mark("start"));
  BpHash none = {nullptr, nullptr, 0, 0};
  hipLaunchKernelGGL(k_bp_column, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, 0, (int64_t)R,
                     (const uint8_t *)h->text.p, h->tab(), col, kind, d_i.p, d_f.p, d_s.p, none, (int64_t *)nullptr, d_ctr.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark(kind == TEHMM_BP_INT ? "ints" : "floats"));
  if (kind == TEHMM_BP_INT) HIPCHK(hipMemcpy(ivalue, d_i.p, R * sizeof(int64_t), hipMemcpyDeviceToHost));
  else HIPCHK(hipMemcpy(fvalue, d_f.p, R * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(status, d_s.p, R, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
  t_bp.host_ints += (int64_t)ctr[2];
  t_bp.host_floats += (int64_t)ctr[3];
  return bp_finish_clock(clk);
}

int tehmm_bed_parse_get_codes(tehmm_bedparse_t *h, int col, int64_t *codes, int64_t *first_records, int64_t *n_distinct,
                              int64_t *n_missing, int64_t *n_empty, int *fell_back) {
  const char *who = "tehmm_bed_parse_get_codes";
  if (!h || h->high > 0) return fail(TEHMM_ERR_ARG, std::string(who) + ": no parse in this handle");
  if (col < 0 || col >= TEHMM_BP_COLS) return fail(TEHMM_ERR_ARG, std::string(who) + ": column 0 to 5");
  if (!n_distinct || !n_missing || !n_empty || !fell_back) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL argument");
  *n_distinct = *n_missing = *n_empty = 0;
  *fell_back = 0;
  const int64_t R = h->records;
  if (R == 0) return TEHMM_OK;
  if (!codes || !first_records) return fail(TEHMM_ERR_ARG, std::string(who) + ": NULL argument");
  uint64_t slots = 1024;
  while (slots < 2 * (uint64_t)R) slots <<= 1;
  DBuf<unsigned long long> d_key, d_first, d_ctr;
  DBuf<int64_t> d_slot, d_rank, d_code, d_frec;
  DBuf<uint32_t> d_isf;
  unsigned long long ctr[TEHMM_BP_CTRS] = {0};
  HIPCHK(d_ctr.upload(ctr, TEHMM_BP_CTRS));
  HIPCHK(d_key.alloc((size_t)slots));
  HIPCHK(d_first.alloc((size_t)slots));
  HIPCHK(d_slot.alloc((size_t)R));
  HIPCHK(d_isf.alloc((size_t)R));
  SegClock clk;
  HIPCHK(clk.mark("start"));
  HIPCHK(hipMemsetAsync(d_key.p, 0, (size_t)slots * sizeof(unsigned long long), 0));
  hipLaunchKernelGGL(k_bp_fill64, dim3(grid_for((int64_t)slots, 256, 1 << 14)), dim3(256), 0, 0, (int64_t)slots, d_first.p,
                     ~0ull);
  BpHash ht = {d_key.p, d_first.p, slots - 1, h->hash_bits};
  const dim3 grid((unsigned)((R + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_bp_column, grid, block, 0, 0, R, (const uint8_t *)h->text.p, h->tab(), col, TEHMM_BP_HASH,
                     (int64_t *)nullptr, (double *)nullptr, (uint8_t *)nullptr, ht, d_slot.p, d_ctr.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("hash"));
  hipLaunchKernelGGL(k_bp_verify, grid, block, 0, 0, R, (const uint8_t *)h->text.p, h->tab(), col, ht,
                     (const int64_t *)d_slot.p, d_isf.p, d_ctr.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("verify"));
  HIPCHK(hipMemcpy(ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
  *n_missing = (int64_t)ctr[4];
  *n_empty = (int64_t)ctr[5];
  if (ctr[6] > 0) {                             // two values behind one hash: the caller's dictionary decides
    *fell_back = 1;
    ++t_bp.code_fallbacks;
    return bp_finish_clock(clk);
  }
  int64_t D = 0;
  int rc = msk_scan(R, d_isf.p, d_rank, &D);
  if (rc != TEHMM_OK) return rc;
  HIPCHK(d_code.alloc((size_t)R));
  HIPCHK(d_frec.alloc((size_t)std::max<int64_t>(D, 1)));
  hipLaunchKernelGGL(k_bp_codes, grid, block, 0, 0, R, ht, (const int64_t *)d_slot.p, (const uint32_t *)d_isf.p,
                     (const int64_t *)d_rank.p, d_code.p, d_frec.p);
  HIPCHK(hipGetLastError());
  HIPCHK(clk.mark("codes"));
  HIPCHK(hipMemcpy(codes, d_code.p, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (D > 0) HIPCHK(hipMemcpy(first_records, d_frec.p, (size_t)D * sizeof(int64_t), hipMemcpyDeviceToHost));
  *n_distinct = D;
  return bp_finish_clock(clk);
}
