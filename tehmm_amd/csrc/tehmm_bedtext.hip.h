// tehmm_bedtext.hip.h -- the per-row BED text of teHmmEval (bin/teHmmEval.py:238-275) formatted on the device
// (DESIGN.md section 5s).  A line is "chrom \t start \t end \t col4 \n"; its length depends on the row alone, so a
// file is a prefix sum over line lengths followed by a byte scatter.
//
// Items: the rows of a list of tables, each table preceded by ONE header item (its optional header line, length 0
// without one): item key[t] = row0[t] + t is table t's header, item key[t] + 1 + i its row i.  A call works through
// the items in stripes.
//
//   k_bt_check_states  names only: lowest row whose state has no name (before the file is touched)
//   k_bt_measure       one lane per item: coordinates as k_bed_coords computes them, digit counts, the length of
//                      column 4; a float64 value is formatted into a 24-byte record (bt_format) or the row is flagged
//   k_bt_patch         the records the host formatted for flagged rows, and their lengths
//   (scan)             k_msk_blocksum, k_tsd_scan_blocks, k_msk_offsets of tehmm_masking.hip.h / tehmm_tsd.hip.h
//   k_bt_emit          a workgroup's 256 items are one contiguous span of the output: lines go to LDS, the span leaves
//                      as aligned 16-byte stores with a ragged head and tail (a span beyond the LDS block: bytes to global)
//
// bt_format: "%.12g" plus ".0" where that text holds only digits.  |x| 10^k, k = 11 - e10, is taken as a double-double
// from a table of 10^k; the 12-digit integer is its nearest, CERTIFIED by the distance of the fraction from 1/2
// against the error bound of the product; anything else is left to the host's snprintf.
#pragma once
#include "tehmm_masking.hip.h"

namespace tehmm {

#define TEHMM_BED_NAMES 0
#define TEHMM_BED_INT 1
#define TEHMM_BED_VALUE 2
#define TEHMM_BT_P10_MIN (-270)          // the table holds 10^k for k in [MIN, MAX]
#define TEHMM_BT_P10_MAX 300
#define TEHMM_BT_REC 24                  // bytes of a value record: text in bytes [0, 23) last character first, length in byte 23
#define TEHMM_BT_LDS 16384               // bytes of a workgroup's staged span
// |computed fraction - true fraction| < 2^-53; a fraction closer than this to 1/2 is not certified
#define TEHMM_BT_MARGIN 9.094947017729282e-13   // 2^-40

struct BtDD {
  double hi, lo;
};

struct BtTable {
  int64_t key;               // item of the table's header: row0 + table index
  int64_t row0, row1;        // rows of the column
  int64_t start, end;        // table_start, table_end
  int64_t seg0;              // first entry of the table's segOffsets in the joined array, -1: unsegmented
  int64_t mask0;             // first entry of its maskOffsets block in the joined array, -1: none
  int32_t chrom_off, chrom_len, hdr_off, hdr_len;      // in the blob
};

struct BtJob {
  const BtTable *tab;
  int n_tables;
  const int64_t *seg;
  const int32_t *mask;
  const uint8_t *blob;
  int kind, shift;
  const int64_t *states;     // column, indexed by row
  const double *values;
  const uint8_t *names;      // names kind: the bytes of all names and where each begins (n_names + 1 entries)
  const int32_t *name_off;
  int n_names;
  const BtDD *pow10;
};

struct BtRec {
  uint64_t t0, t1, t2;       // a 192-bit shift register: the last character pushed is byte 0
  int len;
};

__host__ __device__ __forceinline__ void bt_push(BtRec &r, unsigned c) {
  r.t2 = (r.t2 << 8) | (r.t1 >> 56);
  r.t1 = (r.t1 << 8) | (r.t0 >> 56);
  r.t0 = (r.t0 << 8) | (uint64_t)c;
  ++r.len;
}

// true: r holds the text tehmm_write_bed prints for x; false: not certified here.  (Host and device: the library's
// tehmm_bed_text_format_value runs the same code on the CPU.)
__host__ __device__ inline bool bt_format(double x, const BtDD *pw, BtRec &r) {
  r.t0 = r.t1 = r.t2 = 0;
  r.len = 0;
  uint64_t bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  const bool neg = (bits >> 63) != 0;
  const uint64_t mag = bits & 0x7fffffffffffffffull;
  const int be = (int)(mag >> 52);
  if (be == 0x7ff) {
    if (mag & 0xfffffffffffffull) {
      if (neg) return false;                   // (the C library decides whether that prints a sign)
      bt_push(r, 'n'); bt_push(r, 'a'); bt_push(r, 'n');
      return true;
    }
    if (neg) bt_push(r, '-');
    bt_push(r, 'i'); bt_push(r, 'n'); bt_push(r, 'f');
    return true;
  }
  if (mag == 0) {
    if (neg) bt_push(r, '-');
    bt_push(r, '0'); bt_push(r, '.'); bt_push(r, '0');
    return true;
  }
  if (be == 0) return false;                   // subnormal
  double v;
  __builtin_memcpy(&v, &mag, sizeof(v));
  // floor(log10 v) is floor(e2 log10 2) or one more; the product below says which
  int e10 = ((be - 1023) * 78913) >> 18;
  double hi = 0.0, lo = 0.0;
  bool ok = false;
#pragma unroll 1
  for (int tries = 0; tries < 3 && !ok; ++tries) {
    const int k = 11 - e10;
    if (k < TEHMM_BT_P10_MIN || k > TEHMM_BT_P10_MAX) return false;
    const BtDD P = pw[k - TEHMM_BT_P10_MIN];
    const double p = v * P.hi;
    double e = fma(v, P.hi, -p);               // v P.hi = p + e exactly
    e = fma(v, P.lo, e);
    hi = p + e;
    lo = e - (hi - p);                         // |p| >= |e|: hi + lo = p + e exactly
    if (hi < 1e11) --e10;
    else if (hi >= 1e12) ++e10;
    else ok = true;
  }
  if (!ok) return false;
  double n = rint(hi);
  double fr = (hi - n) + lo;                   // hi - n is exact
  if (fr > 0.5) {
    n += 1.0;
    fr -= 1.0;
  } else if (fr < -0.5) {
    n -= 1.0;
    fr += 1.0;
  }
  if (fabs(fabs(fr) - 0.5) < TEHMM_BT_MARGIN) return false;
  uint64_t D = (uint64_t)n;
  if (D >= 1000000000000ull) {
    D = 100000000000ull;
    ++e10;
  }
  if (D < 100000000000ull) return false;
  // 12 digits as nibbles, the first in bits 44..47
  const uint32_t dh = (uint32_t)(D / 1000000ull), dl = (uint32_t)(D % 1000000ull);
  uint64_t bcd = 0;
  {
    uint32_t a = dh, b = dl;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      bcd |= (uint64_t)(b % 10u) << (4 * q);
      bcd |= (uint64_t)(a % 10u) << (4 * q + 24);
      a /= 10u;
      b /= 10u;
    }
  }
  const int tz = (int)(__builtin_ffsll((long long)bcd) - 1) >> 2;        // bcd != 0
  const int nsig = 12 - tz;
#define BT_DIGIT(j) ('0' + (unsigned)((bcd >> (4 * (11 - (j)))) & 15u))
  if (neg) bt_push(r, '-');
  if (e10 < -4 || e10 >= 12) {
    bt_push(r, BT_DIGIT(0));
    if (nsig > 1) {
      bt_push(r, '.');
      for (int j = 1; j < nsig; ++j) bt_push(r, BT_DIGIT(j));
    }
    bt_push(r, 'e');
    bt_push(r, e10 < 0 ? '-' : '+');
    const unsigned a = (unsigned)(e10 < 0 ? -e10 : e10);
    if (a >= 100u) bt_push(r, '0' + a / 100u);
    bt_push(r, '0' + (a / 10u) % 10u);
    bt_push(r, '0' + a % 10u);
  } else if (e10 >= 0) {
    const int ni = e10 + 1;
    for (int j = 0; j < ni; ++j) bt_push(r, BT_DIGIT(j));
    bt_push(r, '.');
    if (nsig > ni) {
      for (int j = ni; j < nsig; ++j) bt_push(r, BT_DIGIT(j));
    } else {
      bt_push(r, '0');                         // only digits: the ".0" of a Python float
    }
  } else {
    bt_push(r, '0');
    bt_push(r, '.');
    for (int z = 0; z < -e10 - 1; ++z) bt_push(r, '0');
    for (int j = 0; j < nsig; ++j) bt_push(r, BT_DIGIT(j));
  }
#undef BT_DIGIT
  return true;
}

__device__ __forceinline__ int bt_ndigits(uint64_t v) {
  int n = 1;
  if ((v >> 32) == 0) {
    uint32_t w = (uint32_t)v;
    while (w >= 10u) {
      w /= 10u;
      ++n;
    }
    return n;
  }
  while (v >= 10ull) {
    v /= 10ull;
    ++n;
  }
  return n;
}

// characters of a signed integer
__device__ __forceinline__ int bt_int_len(int64_t v) {
  return v < 0 ? 1 + bt_ndigits(0ull - (uint64_t)v) : bt_ndigits((uint64_t)v);
}

__device__ __forceinline__ uint8_t *bt_put_int(uint8_t *dst, int64_t v) {
  uint64_t u = (uint64_t)v;
  if (v < 0) {
    *dst++ = '-';
    u = 0ull - u;
  }
  const int nd = bt_ndigits(u);
  if ((u >> 32) == 0) {
    uint32_t w = (uint32_t)u;
    for (int k = nd - 1; k >= 0; --k) {
      dst[k] = (uint8_t)('0' + w % 10u);
      w /= 10u;
    }
  } else {
    for (int k = nd - 1; k >= 0; --k) {
      dst[k] = (uint8_t)('0' + (unsigned)(u % 10ull));
      u /= 10ull;
    }
  }
  return dst + nd;
}

// the table of item g: the last one whose header item is not behind g
__device__ __forceinline__ int bt_find_table(const BtTable *tab, int n, int64_t g) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid].key <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// start and end of row i of a table: k_bed_coords (tehmm_kernels.hip.h)
__device__ __forceinline__ void bt_coords(const BtJob &job, const BtTable &tb, int64_t i, int64_t *st_out, int64_t *en_out) {
  const int64_t n_rows = tb.row1 - tb.row0;
  int64_t d = i, len = 1;
  if (tb.seg0 >= 0) {
    const int64_t *so = job.seg + tb.seg0;
    d = so[i] - so[0];
    len = i + 1 < n_rows ? so[i + 1] - so[i] : tb.end - (tb.start + so[i]);
  }
  int64_t st = tb.start + d;
  if (tb.mask0 >= 0) st += job.mask[tb.mask0 + d];
  *st_out = st;
  *en_out = st + len;
}

// where row i of a table reads the column (quirk Q15 with shift: one row late, wrapping inside the table)
__device__ __forceinline__ int64_t bt_col_row(const BtJob &job, const BtTable &tb, int64_t i) {
  if (!job.shift) return tb.row0 + i;
  return i == 0 ? tb.row1 - 1 : tb.row0 + i - 1;
}

// viol (preset to ~0): lowest row whose state is outside [0, n_names)
__global__ __launch_bounds__(256) void k_bt_check_states(int64_t n, const int64_t *states, int n_names,
                                                         unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
    if (states[i] < 0 || states[i] >= n_names) atomicMin(viol, (unsigned long long)i);
}

// count[x] = bytes of item i0 + x; values: rec[x] or, for a row that is not certified, its item in flag_item and its
// value in flag_val at slot atomicAdd(ctr) (count[x] then lacks column 4: k_bt_patch adds it)
__global__ __launch_bounds__(256) void k_bt_measure(BtJob job, int64_t i0, int64_t n, uint32_t *count, uint8_t *rec,
                                                    unsigned long long *ctr, uint32_t *flag_item, double *flag_val) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const int64_t g = i0 + x;
  const int t = bt_find_table(job.tab, job.n_tables, g);
  const BtTable tb = job.tab[t];
  if (g == tb.key) {
    count[x] = (uint32_t)tb.hdr_len;
    return;
  }
  const int64_t i = g - tb.key - 1;
  int64_t st, en;
  bt_coords(job, tb, i, &st, &en);
  uint32_t len = (uint32_t)tb.chrom_len + 4u + (uint32_t)bt_int_len(st) + (uint32_t)bt_int_len(en);
  const int64_t c = bt_col_row(job, tb, i);
  if (job.kind == TEHMM_BED_NAMES) {
    const int64_t s = job.states[c];             // (in range: k_bt_check_states)
    len += (uint32_t)(job.name_off[s + 1] - job.name_off[s]);
  } else if (job.kind == TEHMM_BED_INT) {
    len += (uint32_t)bt_int_len(job.states[c]);
  } else {
    const double v = job.values[c];
    BtRec r;
    if (!bt_format(v, job.pow10, r)) {
      r.t0 = r.t1 = r.t2 = 0;
      r.len = 0;
      const unsigned long long slot = atomicAdd(ctr, 1ull);
      flag_item[slot] = (uint32_t)x;
      flag_val[slot] = v;
    }
    uint64_t *q = (uint64_t *)(rec + (size_t)x * TEHMM_BT_REC);
    q[0] = r.t0;
    q[1] = r.t1;
    q[2] = (r.t2 & 0x00ffffffffffffffull) | ((uint64_t)r.len << 56);
    len += (uint32_t)r.len;
  }
  count[x] = len;
}

// the host's text of the flagged rows: recs [n][24] in the record layout
__global__ __launch_bounds__(256) void k_bt_patch(int64_t n, const uint32_t *flag_item, const uint8_t *recs, uint32_t *count,
                                                  uint8_t *rec) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const uint32_t x = flag_item[s];
  const uint64_t *src = (const uint64_t *)(recs + (size_t)s * TEHMM_BT_REC);
  uint64_t *q = (uint64_t *)(rec + (size_t)x * TEHMM_BT_REC);
  q[0] = src[0];
  q[1] = src[1];
  q[2] = src[2];
  count[x] += (uint32_t)(src[2] >> 56);
}

// the text of item g at dst
__device__ __forceinline__ void bt_line(const BtJob &job, int64_t g, uint8_t *dst, const uint8_t *rec) {
  const int t = bt_find_table(job.tab, job.n_tables, g);
  const BtTable tb = job.tab[t];
  if (g == tb.key) {
    const uint8_t *h = job.blob + tb.hdr_off;
    for (int q = 0; q < tb.hdr_len; ++q) dst[q] = h[q];
    return;
  }
  const int64_t i = g - tb.key - 1;
  const uint8_t *ch = job.blob + tb.chrom_off;
  for (int q = 0; q < tb.chrom_len; ++q) dst[q] = ch[q];
  dst += tb.chrom_len;
  int64_t st, en;
  bt_coords(job, tb, i, &st, &en);
  *dst++ = '\t';
  dst = bt_put_int(dst, st);
  *dst++ = '\t';
  dst = bt_put_int(dst, en);
  *dst++ = '\t';
  const int64_t c = bt_col_row(job, tb, i);
  if (job.kind == TEHMM_BED_NAMES) {
    const int64_t s = job.states[c];
    const int a = job.name_off[s], b = job.name_off[s + 1];
    for (int q = a; q < b; ++q) *dst++ = job.names[q];
  } else if (job.kind == TEHMM_BED_INT) {
    dst = bt_put_int(dst, job.states[c]);
  } else {
    const uint64_t *q = (const uint64_t *)rec;
    const uint64_t t0 = q[0], t1 = q[1], t2 = q[2];
    const int len = (int)(t2 >> 56);
    for (int k = len - 1; k >= 0; --k) {
      const uint64_t w = k < 8 ? t0 : k < 16 ? t1 : t2;
      *dst++ = (uint8_t)(w >> (8 * (k & 7)));
    }
  }
  *dst = '\n';
}

// out: the stripe's text, 16-byte aligned; off: exclusive scan of count; total: the stripe's bytes
__global__ __launch_bounds__(256) void k_bt_emit(BtJob job, int64_t i0, int64_t n, const int64_t *off, const int64_t *total,
                                                 const uint8_t *rec, uint8_t *out) {
  __shared__ __attribute__((aligned(16))) uint8_t sh[TEHMM_BT_LDS + 16];
  const int64_t first = (int64_t)blockIdx.x * 256;
  const int64_t last = first + 256 < n ? first + 256 : n;
  const int64_t x = first + threadIdx.x;
  const int64_t span0 = off[first], span1 = last < n ? off[last] : *total;
  const int64_t span = span1 - span0;
  const bool mine = x < last;
  const int64_t o = mine ? off[x] : 0;
  const int64_t o1 = mine ? (x + 1 < n ? off[x + 1] : *total) : 0;
  const uint8_t *myrec = rec ? rec + (size_t)x * TEHMM_BT_REC : nullptr;
  if (span > TEHMM_BT_LDS) {                   // long names or headers: straight to memory
    if (mine && o1 > o) bt_line(job, i0 + x, out + o, myrec);
    return;
  }
  // LDS byte q is output byte base + q, base = span0 rounded down to 16
  const int head = (int)(span0 & 15);
  const int64_t base = span0 - head;
  if (mine && o1 > o) bt_line(job, i0 + x, sh + (int)(o - span0) + head, myrec);
  __syncthreads();
  const int end = head + (int)span;
  for (int q = (int)threadIdx.x * 16; q < end; q += 256 * 16) {
    if (q >= head && q + 16 <= end) {
      *(uint4 *)(out + base + q) = *(const uint4 *)(sh + q);
    } else {
      const int a = q > head ? q : head, b = q + 16 < end ? q + 16 : end;
      for (int j = a; j < b; ++j) out[base + j] = sh[j];
    }
  }
}

}  // namespace tehmm
