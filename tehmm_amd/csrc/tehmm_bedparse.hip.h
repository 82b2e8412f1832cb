// tehmm_bedparse.hip.h -- BED text parsed on the device (trackIO.bedRead and what BedFile builds from it; DESIGN.md
// section 5u).  The rule is bedRead's: lines end at "\n", "\r\n" or a lone "\r" (a last line without a terminator
// counts), a line whose first byte is '#' is dropped, fields are split on tabs, a line with fewer than three fields is
// dropped.
//
//   k_bp_classify   one lane per 16 bytes (one uint4 load), a workgroup per tile of TEHMM_BP_TILE bytes: a bit per byte
//                   for "a line ends here" (a "\n", a "\r" whose NEXT byte is no "\n", the file's last byte) and one for
//                   "tab", both kept as one 32-bit word per 16 bytes; the tile's number of line ends; bytes >= 0x80
//   (scan)          k_msk_blocksum, k_tsd_scan_blocks, k_msk_offsets over the tile counts (64-bit)
//   k_bp_lines      from the masks alone: the position of every line end, in file order
//   k_bp_keep       one lane per line: its first byte and, from the tab masks, whether it has three fields
//   (scan)          over the keep flags: the record index of every kept line
//   k_bp_fields     a workgroup's 256 lines are one contiguous span of the text: it goes to LDS with 16-byte loads, and
//                   every lane walks ITS line there: field offsets and lengths of columns 0..5, the field count, the
//                   integers of columns 1 and 2 (a span beyond the LDS block: bytes from global memory, the slow path)
//   k_bp_column     the same staging over 256 records: the integer, the float or the hash-table slot of one column
//   k_bp_verify     every record's field against its slot's first record, byte for byte; marks the first records
//   k_bp_codes      code = rank of the slot's first record among the first records (order of first appearance)
//
// bp_parse_int / bp_parse_float are __host__ __device__: tehmm_bed_parse_number runs them on the CPU.  They certify
// [+-]?[0-9]{1,18} and the classical exact float case (at most 15 significant digits, |e10| <= 22: one correctly
// rounded multiplication or division of two exact doubles); everything else is left to the host's int() / float().
#pragma once
#include "tehmm_masking.hip.h"

namespace tehmm {

#define TEHMM_BP_TILE 4096               // bytes a workgroup classifies: 256 lanes x 16
#define TEHMM_BP_LDS 32768               // bytes of a record workgroup's staged span
#define TEHMM_BP_COLS 6                  // columns of the field table
#define TEHMM_BP_PAD 48                  // zero bytes behind the text (the classify lane's next byte, the staging loads)
#define TEHMM_BP_INT 0
#define TEHMM_BP_FLOAT 1
#define TEHMM_BP_HASH 2
#define TEHMM_BP_CERTIFIED 0             // status bytes
#define TEHMM_BP_HOST 1
#define TEHMM_BP_MISSING 2

// [+-]?[0-9]{1,18}
__host__ __device__ inline bool bp_parse_int(const uint8_t *p, int64_t len, int64_t *out) {
  int64_t i = 0;
  bool neg = false;
  if (len > 0 && (p[0] == '+' || p[0] == '-')) {
    neg = p[0] == '-';
    i = 1;
  }
  const int64_t nd = len - i;
  if (nd < 1 || nd > 18) return false;
  uint64_t v = 0;
  for (; i < len; ++i) {
    const unsigned d = (unsigned)p[i] - (unsigned)'0';
    if (d > 9u) return false;
    v = v * 10u + d;
  }
  *out = neg ? -(int64_t)v : (int64_t)v;
  return true;
}

// [+-]? digits with at most one '.' (at least one digit) ([eE][+-]?digits)?; significant digits: from the first
// non-zero digit to the last digit of the mantissa, at most 15; e10 = exponent - fraction digits, |e10| <= 22.
// A mantissa of zeros is +-0.0 whatever the exponent says.
__host__ __device__ inline bool bp_parse_float(const uint8_t *p, int64_t len, double *out) {
  int64_t i = 0;
  bool neg = false;
  if (len > 0 && (p[0] == '+' || p[0] == '-')) {
    neg = p[0] == '-';
    i = 1;
  }
  uint64_t w = 0;
  int nsig = 0, ndig = 0, frac = 0;
  bool point = false;
  for (; i < len; ++i) {
    const unsigned c = p[i];
    const unsigned d = c - (unsigned)'0';
    if (d <= 9u) {
      ++ndig;
      if (point) ++frac;
      if (nsig > 0 || d != 0u) {
        if (++nsig > 15) return false;
        w = w * 10u + d;
      }
      if (frac > 100000) return false;
    } else if (c == '.' && !point) {
      point = true;
    } else {
      break;
    }
  }
  if (ndig == 0) return false;
  int ex = 0;
  if (i < len) {
    if (p[i] != 'e' && p[i] != 'E') return false;
    ++i;
    bool eneg = false;
    if (i < len && (p[i] == '+' || p[i] == '-')) {
      eneg = p[i] == '-';
      ++i;
    }
    if (i >= len) return false;
    for (; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - (unsigned)'0';
      if (d > 9u) return false;
      if (ex < 1000000) ex = ex * 10 + (int)d;
    }
    if (eneg) ex = -ex;
  }
  double v = 0.0;
  if (w != 0) {
    const int e10 = ex - frac;
    if (e10 < -22 || e10 > 22) return false;
    double pw = 1.0;                              // 10^k, k <= 22: every product is exact
    const int a = e10 < 0 ? -e10 : e10;
    for (int k = 0; k < a; ++k) pw *= 10.0;
    v = e10 < 0 ? (double)w / pw : (double)w * pw;
  }
  *out = neg ? -v : v;
  return true;
}

// 64-bit FNV-1a and a finishing mix; bit 63 is set so that no key is 0 (the empty slot); hash_bits truncates (tests)
__host__ __device__ inline uint64_t bp_hash(const uint8_t *p, int64_t len, int hash_bits) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int64_t i = 0; i < len; ++i) h = (h ^ (uint64_t)p[i]) * 0x100000001b3ull;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  if (hash_bits < 63) h &= (1ull << hash_bits) - 1ull;
  return h | (1ull << 63);
}

// ctr: [0] bytes >= 0x80, [1] lines beyond 2^31 - 1 bytes, [2] integers left to the host, [3] floats left to the host,
//      [4] records without the column, [5] empty values, [6] fields that differ from their slot's first record
#define TEHMM_BP_CTRS 8

__global__ __launch_bounds__(256) void k_bp_classify(const uint8_t *text, int64_t n, uint32_t *mask, uint32_t *count,
                                                     unsigned long long *ctr) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t b0 = c * 16;
  uint32_t ends = 0, tabs = 0, high = 0;
  if (b0 < n) {
    const uint4 v = *(const uint4 *)(text + b0);         // (zeros behind byte n - 1)
    const uint32_t next = text[b0 + 16];                 // the neighbour lane's, wave's or workgroup's first byte
    const uint32_t w[5] = {v.x, v.y, v.z, v.w, next};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 255u;
      const uint32_t nb = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u;
      const bool end = b == '\n' || (b == '\r' && nb != '\n') || b0 + j == n - 1;
      if (b0 + j < n) {
        ends |= (end ? 1u : 0u) << j;
        tabs |= (b == '\t' ? 1u : 0u) << j;
        high |= b & 128u;
      }
    }
    mask[c] = ends | (tabs << 16);
  }
  if (high) atomicAdd(ctr, 1ull);
  int64_t total;
  msk_block_excl((int64_t)__popc(ends), &total);
  if (threadIdx.x == 0) count[blockIdx.x] = (uint32_t)total;
}

// lend[i] = position of the last byte of line i (its terminator's last byte, or the file's last byte)
__global__ __launch_bounds__(256) void k_bp_lines(int64_t n_chunks, const uint32_t *mask, const int64_t *tile_off,
                                                  int64_t *lend) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t ends = c < n_chunks ? mask[c] & 0xffffu : 0u;
  int64_t at = tile_off[blockIdx.x] + msk_block_excl((int64_t)__popc(ends), nullptr);
  while (ends) {
    const int j = __builtin_ctz(ends);
    ends &= ends - 1u;
    lend[at++] = c * 16 + j;
  }
}

// where line i begins, and where its text ends (the terminator taken off)
__device__ __forceinline__ void bp_line_span(const uint8_t *text, const int64_t *lend, int64_t i, int64_t *s_out,
                                             int64_t *ce_out) {
  const int64_t s = i > 0 ? lend[i - 1] + 1 : 0, e = lend[i];
  const uint8_t last = text[e];
  int64_t ce = e + 1;
  if (last == '\n') {
    ce = e;
    if (ce > s && text[e - 1] == '\r') --ce;
  } else if (last == '\r') {
    ce = e;
  }
  *s_out = s;
  *ce_out = ce;
}

// keep[i] = 1: line i is a record (no '#' in front, at least two tabs in its text)
__global__ __launch_bounds__(256) void k_bp_keep(int64_t n_lines, const uint8_t *text, const uint32_t *mask,
                                                 const int64_t *lend, uint32_t *keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_lines) return;
  int64_t s, ce;
  bp_line_span(text, lend, i, &s, &ce);
  uint32_t k = 0;
  if (text[s] != '#' && ce > s) {
    int tabs = 0;
    for (int64_t c = s >> 4; c <= (ce - 1) >> 4 && tabs < 2; ++c) {
      uint32_t t = mask[c] >> 16;
      const int64_t b0 = c * 16;
      if (b0 < s) t &= 0xffffu << (int)(s - b0);
      if (b0 + 16 > ce) t &= 0xffffu >> (int)(b0 + 16 - ce);
      tabs += __popc(t);
    }
    k = tabs >= 2 ? 1u : 0u;
  }
  keep[i] = k;
}

// The bytes [first, last) of the text for a workgroup: in LDS when they fit (*org = the text position of src[0]),
// otherwise the text itself.  Every thread of the workgroup calls it.
__device__ __forceinline__ const uint8_t *bp_stage(const uint8_t *text, int64_t first, int64_t last, uint8_t *sh,
                                                   int64_t *org) {
  const int64_t base = first & ~(int64_t)15;
  if (last - base > TEHMM_BP_LDS) {
    *org = 0;
    return text;
  }
  const int span = (int)(last - base);
  for (int q = (int)threadIdx.x * 16; q < span; q += 256 * 16) *(uint4 *)(sh + q) = *(const uint4 *)(text + base + q);
  __syncthreads();
  *org = base;
  return sh;
}

struct BpTable {
  int64_t *line_start, *line_len;      // [records]
  int32_t *n_fields;                   // [records]
  int32_t *field_off, *field_len;      // [records][TEHMM_BP_COLS], offsets from the line's start, length -1: no column
  int64_t *ival[2];                    // columns 1 and 2
  uint8_t *istat[2];
};

__global__ __launch_bounds__(256) void k_bp_fields(int64_t n_lines, const uint8_t *text, const int64_t *lend,
                                                   const uint32_t *keep, const int64_t *rec_of, BpTable tab,
                                                   unsigned long long *ctr) {
  __shared__ __attribute__((aligned(16))) uint8_t sh[TEHMM_BP_LDS];
  const int64_t l0 = (int64_t)blockIdx.x * 256;
  const int64_t l1 = l0 + 256 < n_lines ? l0 + 256 : n_lines;
  const int64_t first = l0 > 0 ? lend[l0 - 1] + 1 : 0, last = lend[l1 - 1] + 1;
  int64_t org;
  const uint8_t *src = bp_stage(text, first, last, sh, &org);
  const int64_t i = l0 + threadIdx.x;
  if (i >= l1 || !keep[i]) return;
  int64_t s, ce;
  bp_line_span(text, lend, i, &s, &ce);
  const int64_t r = rec_of[i];
  const uint8_t *p = src + (s - org);
  const int64_t len = ce - s;
  if (len > 0x7fffffff) {
    atomicAdd(ctr + 1, 1ull);
    return;
  }
  int32_t off[TEHMM_BP_COLS], fl[TEHMM_BP_COLS];
#pragma unroll
  for (int k = 0; k < TEHMM_BP_COLS; ++k) {
    off[k] = 0;
    fl[k] = -1;
  }
  int nf = 0;
  int32_t f0 = 0;
  for (int32_t q = 0; q <= (int32_t)len; ++q) {
    if (q == (int32_t)len || p[q] == '\t') {
#pragma unroll
      for (int k = 0; k < TEHMM_BP_COLS; ++k)
        if (k == nf) {
          off[k] = f0;
          fl[k] = q - f0;
        }
      ++nf;
      f0 = q + 1;
    }
  }
  tab.line_start[r] = s;
  tab.line_len[r] = len;
  tab.n_fields[r] = nf;
#pragma unroll
  for (int k = 0; k < TEHMM_BP_COLS; ++k) {
    tab.field_off[r * TEHMM_BP_COLS + k] = off[k];
    tab.field_len[r * TEHMM_BP_COLS + k] = fl[k];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {                  // (a record has columns 1 and 2)
    int64_t v = 0;
    const bool ok = bp_parse_int(p + off[k + 1], fl[k + 1], &v);
    tab.ival[k][r] = v;
    tab.istat[k][r] = ok ? TEHMM_BP_CERTIFIED : TEHMM_BP_HOST;
    if (!ok) atomicAdd(ctr + 2, 1ull);
  }
}

struct BpHash {
  unsigned long long *key, *first;     // [slots]: 0 = empty; the lowest record that hashed into the slot
  uint64_t slot_mask;                  // slots - 1 (a power of two)
  int hash_bits;
};

// kind INT / FLOAT: ival or fval, stat.  kind HASH: slot (-1: no such column) of the record's field in the table
__global__ __launch_bounds__(256) void k_bp_column(int64_t n_rec, const uint8_t *text, BpTable tab, int col, int kind,
                                                   int64_t *ival, double *fval, uint8_t *stat, BpHash ht, int64_t *slot,
                                                   unsigned long long *ctr) {
  __shared__ __attribute__((aligned(16))) uint8_t sh[TEHMM_BP_LDS];
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  const int64_t r1 = r0 + 256 < n_rec ? r0 + 256 : n_rec;
  int64_t org;
  const uint8_t *src = bp_stage(text, tab.line_start[r0], tab.line_start[r1 - 1] + tab.line_len[r1 - 1], sh, &org);
  const int64_t r = r0 + threadIdx.x;
  if (r >= r1) return;
  const int32_t fl = tab.field_len[r * TEHMM_BP_COLS + col];
  const uint8_t *p = src + (tab.line_start[r] + tab.field_off[r * TEHMM_BP_COLS + col] - org);
  if (kind == TEHMM_BP_HASH) {
    if (fl < 0) {
      slot[r] = -1;
      atomicAdd(ctr + 4, 1ull);
      return;
    }
    if (fl == 0) atomicAdd(ctr + 5, 1ull);
    const unsigned long long h = bp_hash(p, fl, ht.hash_bits);
    uint64_t q = (h ^ (h >> 29)) & ht.slot_mask;
    for (;;) {                                   // (slots >= 2 records: there is always an empty one)
      unsigned long long k = ht.key[q];
      if (k == 0ull) k = atomicCAS(ht.key + q, 0ull, h);
      if (k == 0ull || k == h) break;
      q = (q + 1) & ht.slot_mask;
    }
    if (ht.first[q] > (unsigned long long)r) atomicMin(ht.first + q, (unsigned long long)r);
    slot[r] = (int64_t)q;
    return;
  }
  if (fl < 0) {
    stat[r] = TEHMM_BP_MISSING;
    if (kind == TEHMM_BP_INT) ival[r] = 0;
    else fval[r] = 0.0;
    atomicAdd(ctr + 4, 1ull);
    return;
  }
  bool ok;
  if (kind == TEHMM_BP_INT) {
    int64_t v = 0;
    ok = bp_parse_int(p, fl, &v);
    ival[r] = v;
    if (!ok) atomicAdd(ctr + 2, 1ull);
  } else {
    double v = 0.0;
    ok = bp_parse_float(p, fl, &v);
    fval[r] = v;
    if (!ok) atomicAdd(ctr + 3, 1ull);
  }
  stat[r] = ok ? TEHMM_BP_CERTIFIED : TEHMM_BP_HOST;
}

// is_first[r] = 1: record r is the first of its value.  A record whose bytes differ from its slot's first record
// (two values, one hash) is counted: the column then goes to the host dictionary.
__global__ __launch_bounds__(256) void k_bp_verify(int64_t n_rec, const uint8_t *text, BpTable tab, int col, BpHash ht,
                                                   const int64_t *slot, uint32_t *is_first, unsigned long long *ctr) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const int64_t q = slot[r];
  if (q < 0) {
    is_first[r] = 0;
    return;
  }
  const int64_t f = (int64_t)ht.first[q];
  is_first[r] = f == r ? 1u : 0u;
  if (f == r) return;
  const int32_t la = tab.field_len[r * TEHMM_BP_COLS + col], lb = tab.field_len[f * TEHMM_BP_COLS + col];
  bool same = la == lb;
  if (same) {
    const uint8_t *a = text + tab.line_start[r] + tab.field_off[r * TEHMM_BP_COLS + col];
    const uint8_t *b = text + tab.line_start[f] + tab.field_off[f * TEHMM_BP_COLS + col];
    for (int32_t x = 0; x < la && same; ++x) same = a[x] == b[x];
  }
  if (!same) atomicAdd(ctr + 6, 1ull);
}

// rank = exclusive scan of is_first: code[r] = rank of the value's first record; first_rec[rank] = that record
__global__ __launch_bounds__(256) void k_bp_codes(int64_t n_rec, BpHash ht, const int64_t *slot, const uint32_t *is_first,
                                                  const int64_t *rank, int64_t *code, int64_t *first_rec) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const int64_t q = slot[r];
  if (q < 0) {
    code[r] = -1;
    return;
  }
  code[r] = rank[(int64_t)ht.first[q]];
  if (is_first[r]) first_rec[rank[r]] = r;
}

__global__ __launch_bounds__(256) void k_bp_fill64(int64_t n, unsigned long long *p, unsigned long long v) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) p[i] = v;
}

}  // namespace tehmm
