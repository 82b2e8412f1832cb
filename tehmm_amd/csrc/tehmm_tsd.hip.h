// tehmm_tsd.hip.h -- the target-site-duplication finder (bin/tsdFinder.py on kmer.py) and the overlap clean-up of
// bin/removeBedOverlaps.py as device kernels.
//
// An element (sequence, start, end) has a query window left of it and a table window right of it, each at most
// TEHMM_TSD_WINDOW bases.  One lane owns one element.  It keeps both windows as five 64-bit position masks, one per
// symbol (a, c, g, t, n), and walks the diagonals j - i = d of the (query, table) grid: the base-equality mask of a
// diagonal is five ANDs of a query mask with a shifted table mask, its k-mer hits are k - 1 shifted ANDs of that, and
// every run of R consecutive hits gives the pieces the reference's greedy list merge ends with: one at every `per`-th
// hit of the run, k + min(per - 1, hits behind it in the run) long.  Nothing is a list: the cost of an element is
// bounded by its window sizes, however repetitive the bases are.
//
//   k_tsd_find        validity of the window bases, matches per element, the selected match (d, then L, then i, j)
//   k_tsd_blocksum, k_tsd_scan_blocks, k_tsd_offsets      exclusive 64-bit scan of the counts
//   k_tsd_scatter     the matches in the reference's list order (i, then j) at their element's offset
//   k_rmo_*           removeBedOverlaps: segmented running maximum of the ends, then the segmenter's compaction
#pragma once
#include "tehmm_segment.hip.h"

namespace tehmm {

#define TEHMM_TSD_WINDOW 64      // bases of a search window: one bit each of a 64-bit mask
#define TEHMM_TSD_MAX_K 21       // hashDNA (kmer.py:20) asserts above it

struct TsdOpt {
  int k, left, right, overlap;      // overlap >= 0
  int per;                          // hits of a full piece: max(k, max - k) - k + 1, at most TEHMM_TSD_WINDOW
  int max_score;                    // -1: no filter
  int all;
};

struct TsdElems {
  int64_t n;
  const int32_t *seq;               // [n] sequence of the element
  const int64_t *start, *end;       // [n]
  const int64_t *seq_off;           // [n_seq + 1] into bases
  const uint8_t *bases;             // padded: reading the aligned 8 bytes around any base is inside the buffer
};

struct TsdWin {
  int64_t l1, l2;                   // first base of the query / table window, inside the sequence
  int m, w;                         // their lengths, k <= m, w <= TEHMM_TSD_WINDOW
};

// the windows of intervalTsds (tsdFinder.py:245-254); false when the element yields nothing
__device__ inline bool tsd_windows(const TsdOpt &o, int64_t s, int64_t e, int64_t len, TsdWin &W) {
  int64_t ov = (e - s) / 2 - 2;
  if (ov > o.overlap) ov = o.overlap;
  if (ov < 0) ov = 0;
  const int64_t l2 = e - ov;
  if (l2 >= len) return false;      // (r2 <= len - 1: nothing to search; also keeps e + right from overflowing)
  const int64_t l1 = s - o.left > 0 ? s - (int64_t)o.left : 0;
  const int64_t r1 = s - 1 + ov;
  const int64_t r2 = e - 1 + o.right < len - 1 ? e - 1 + (int64_t)o.right : len - 1;
  const int64_t m = r1 - l1, w = r2 - l2;
  if (m < o.k || w < o.k || m > TEHMM_TSD_WINDOW || w > TEHMM_TSD_WINDOW) return false;
  W.l1 = l1;
  W.l2 = l2;
  W.m = (int)m;
  W.w = (int)w;
  return true;
}

// position masks of bases[a, a + len), len <= 64, case folded; false when a base is none of acgtn
__device__ inline bool tsd_planes(const uint8_t *bases, int64_t a, int len, uint64_t P[5]) {
  P[0] = P[1] = P[2] = P[3] = P[4] = 0;
  bool ok = true;
  const int64_t b = a + len;
  for (int64_t w0 = a & ~7ll; w0 < b; w0 += 8) {
    const uint64_t v = *reinterpret_cast<const uint64_t *>(bases + w0);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int64_t pos = w0 + t;
      if (pos < a || pos >= b) continue;
      const unsigned ch = ((unsigned)(v >> (8 * t)) & 0xffu) | 0x20u;
      const uint64_t bit = 1ull << (int)(pos - a);
      if (ch == 'a') P[0] |= bit;
      else if (ch == 'c') P[1] |= bit;
      else if (ch == 'g') P[2] |= bit;
      else if (ch == 't') P[3] |= bit;
      else if (ch == 'n') P[4] |= bit;
      else ok = false;
    }
  }
  return ok;
}

// f(i, j, L) for every piece, diagonals ascending (so within a query position i the table positions j ascend)
template <class F>
__device__ inline void tsd_pieces(const TsdOpt &o, const uint64_t Q[5], const uint64_t C[5], int m, int w, F f) {
  const int k = o.k, per = o.per;
  for (int d = k - m; d <= w - k; ++d) {
    uint64_t E = 0;                                       // bit i: query base i equals table base i + d
#pragma unroll
    for (int a = 0; a < 5; ++a) E |= Q[a] & (d >= 0 ? C[a] >> d : C[a] << -d);
    uint64_t H = E;                                       // bit i: the k-mers at (i, i + d) are equal
    for (int t = 1; t < k && H; ++t) H &= E >> t;
    while (H) {
      const int i0 = __builtin_ctzll(H);
      const uint64_t x = ~(H >> i0);
      const int R = x ? __builtin_ctzll(x) : 64;          // hits of this run
      H = i0 + R >= 64 ? 0ull : H & (~0ull << (i0 + R));
      for (int off = 0; off < R; off += per) {
        const int rest = R - 1 - off;
        f(i0 + off, i0 + off + d, k + (rest < per - 1 ? rest : per - 1));
      }
    }
  }
}

// the selection of tsdFinder.py:275-287 as one minimum: d, then the longer match, then list order (i, then j)
__device__ inline uint32_t tsd_key(int d, int L, int i, int j) {
  return ((uint32_t)d << 19) | ((uint32_t)(TEHMM_TSD_WINDOW - L) << 12) | ((uint32_t)i << 6) | (uint32_t)j;
}

struct TsdElem {
  int64_t s, e, base;      // base: offset of the element's sequence in bases
  TsdWin W;
};

__device__ inline bool tsd_elem(const TsdElems &el, const TsdOpt &o, int64_t x, TsdElem &E) {
  const int32_t si = el.seq[x];
  E.s = el.start[x];
  E.e = el.end[x];
  E.base = el.seq_off[si];
  return tsd_windows(o, E.s, E.e, el.seq_off[si + 1] - E.base, E.W);
}

__device__ inline int tsd_abs(int64_t v) { return (int)(v < 0 ? -v : v); }

// d1, d2 of getScore (tsdFinder.py:234-240)
__device__ inline void tsd_score(const TsdElem &E, int i, int j, int L, int &d1, int &d2) {
  d1 = tsd_abs(E.s - (E.W.l1 + i + L));
  d2 = tsd_abs(E.e - (E.W.l2 + j));
}

// count[x]: matches of element x that pass maxScore (without all: 0 or 1); best[x]: tsd_key of the selected one;
// viol (preset to ~0): lowest element with a base outside acgtn in a searched window (its count is 0)
__global__ __launch_bounds__(256) void k_tsd_find(TsdElems el, TsdOpt o, int32_t *count, uint32_t *best,
                                                  unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < el.n; x += step) {
    TsdElem E;
    int cnt = 0;
    uint32_t key = ~0u;
    if (tsd_elem(el, o, x, E)) {
      uint64_t Q[5], C[5];
      const bool okq = tsd_planes(el.bases, E.base + E.W.l1, E.W.m, Q);
      const bool okc = tsd_planes(el.bases, E.base + E.W.l2, E.W.w, C);
      if (!okq || !okc) atomicMin(viol, (unsigned long long)x);
      else
        tsd_pieces(o, Q, C, E.W.m, E.W.w, [&](int i, int j, int L) {
          int d1, d2;
          tsd_score(E, i, j, L, d1, d2);
          const int d = d1 > d2 ? d1 : d2;
          if (o.max_score != -1 && d > o.max_score) return;
          ++cnt;
          const uint32_t kk = tsd_key(d, L, i, j);
          key = kk < key ? kk : key;
        });
    }
    count[x] = o.all ? cnt : (cnt ? 1 : 0);
    best[x] = key;
  }
}

// ---- exclusive scan of the counts, 64 bits across workgroups ------------------------------------------------------
__global__ __launch_bounds__(256) void k_tsd_blocksum(int64_t n, const int32_t *count, int64_t *block_sum) {
  __shared__ unsigned wsum[4];
  const int64_t base = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK;
  unsigned c = 0;                                         // at most 2048 x 4096
  for (int q = 0; q < 8; ++q) {
    const int64_t i = base + q * 256 + threadIdx.x;
    if (i < n) c += (unsigned)count[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_sum[blockIdx.x] = (int64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of the block sums in place (one workgroup), the total in *total
__global__ __launch_bounds__(256) void k_tsd_scan_blocks(int64_t n_blocks, int64_t *block_sum, int64_t *total) {
  __shared__ int64_t sh[256];
  __shared__ int64_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < n_blocks; b0 += 256) {
    const int64_t i = b0 + threadIdx.x;
    const int64_t v = i < n_blocks ? block_sum[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int64_t add = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    const int64_t incl = sh[threadIdx.x], carry = carry_s;
    if (i < n_blocks) block_sum[i] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == 255) carry_s = carry + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry_s;
}

// off[x] = matches of all elements before x; thread t owns the 8 consecutive elements base + 8 t ..
__global__ __launch_bounds__(256) void k_tsd_offsets(int64_t n, const int32_t *count, const int64_t *block_sum,
                                                     int64_t *off) {
  __shared__ unsigned wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  unsigned c[8], mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = i0 + q < n ? (unsigned)count[i0 + q] : 0u;
    mine += c[q];
  }
  unsigned incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  int64_t before = block_sum[blockIdx.x] + (int64_t)(incl - mine);
  for (int q = 0; q < w; ++q) before += wtot[q];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (i0 + q < n) off[i0 + q] = before;
    before += c[q];
  }
}

struct TsdOut {
  int64_t cap;                       // rows of the six columns
  int64_t *ls, *le, *d1, *rs, *re, *d2;
};

__device__ inline void tsd_emit(const TsdOut &out, int64_t r, const TsdElem &E, int i, int j, int L) {
  if (r < 0 || r >= out.cap) return;
  int d1, d2;
  tsd_score(E, i, j, L, d1, d2);
  out.ls[r] = E.W.l1 + i;
  out.le[r] = E.W.l1 + i + L;
  out.d1[r] = d1;
  out.rs[r] = E.W.l2 + j;
  out.re[r] = E.W.l2 + j + L;
  out.d2[r] = d2;
}

// Without ALL the selected match of k_tsd_find is decoded.  With ALL the pieces are found again, twice: once to count
// them per query position (64 counters per lane in LDS, column tid), once to place them; since the diagonals
// ascend, the pieces of one query position come in ascending j, so "start of the row + pieces of the row so far" is
// the rank in the reference's list order.
template <bool ALL>
__global__ __launch_bounds__(256) void k_tsd_scatter(TsdElems el, TsdOpt o, const int32_t *count, const uint32_t *best,
                                                     const int64_t *off, TsdOut out) {
  __shared__ uint16_t rows[ALL ? TEHMM_TSD_WINDOW * 256 : 1];
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < el.n; x += step) {
    if (count[x] <= 0) continue;
    TsdElem E;
    if (!tsd_elem(el, o, x, E)) continue;
    if (!ALL) {
      const uint32_t key = best[x];
      tsd_emit(out, off[x], E, (int)((key >> 6) & 63u), (int)(key & 63u),
               TEHMM_TSD_WINDOW - (int)((key >> 12) & 127u));
      continue;
    }
    uint64_t Q[5], C[5];
    tsd_planes(el.bases, E.base + E.W.l1, E.W.m, Q);
    tsd_planes(el.bases, E.base + E.W.l2, E.W.w, C);
    uint16_t *row = rows + threadIdx.x;
    for (int i = 0; i < E.W.m; ++i) row[i * 256] = 0;
    auto kept = [&](int i, int j, int L) {
      int d1, d2;
      tsd_score(E, i, j, L, d1, d2);
      return o.max_score == -1 || (d1 > d2 ? d1 : d2) <= o.max_score;
    };
    tsd_pieces(o, Q, C, E.W.m, E.W.w, [&](int i, int j, int L) {
      if (kept(i, j, L)) ++row[i * 256];
    });
    unsigned run = 0;
    for (int i = 0; i < E.W.m; ++i) {
      const unsigned c = row[i * 256];
      row[i * 256] = (uint16_t)run;
      run += c;
    }
    const int64_t at = off[x];
    tsd_pieces(o, Q, C, E.W.m, E.W.w, [&](int i, int j, int L) {
      if (kept(i, j, L)) tsd_emit(out, at + row[i * 256]++, E, i, j, L);
    });
  }
}

// ---- removeBedOverlaps.py:76-95 on a list sorted by (chrom, start) ---------------------------------------------------
// The chain "start = max(start, end of the last kept interval of the chromosome); keep iff end > start" never needs
// the kept set: a dropped interval ends at or before the last kept end or at or before its own start, which no later
// start undercuts, so the last kept end is the maximum of ALL earlier ends of the chromosome.  That is a segmented
// scan with the operator (c1, m1) . (c2, m2) = c1 == c2 ? (c2, max(m1, m2)) : (c2, m2).

// viol (preset to ~0): lowest i whose chrom id is below its predecessor's, or whose start is on the same chrom
__global__ __launch_bounds__(256) void k_rmo_check(int64_t n, const int32_t *chrom, const int64_t *start,
                                                   unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; i < n; i += step) {
    const int32_t c = chrom[i], cp = chrom[i - 1];
    if (c < cp || (c == cp && start[i] < start[i - 1])) atomicMin(viol, (unsigned long long)i);
  }
}

struct RmoAgg {
  int32_t c;
  int64_t m;      // INT64_MIN: nothing
};

__device__ inline RmoAgg rmo_join(const RmoAgg &a, const RmoAgg &b) {
  RmoAgg r = b;
  if (a.c == b.c && a.m > b.m) r.m = a.m;
  return r;
}

__device__ inline RmoAgg rmo_shfl_up(const RmoAgg &a, int o) {
  RmoAgg r;
  r.c = __shfl_up(a.c, o);
  const int lo = __shfl_up((int)(uint32_t)(uint64_t)a.m, o), hi = __shfl_up((int)((uint64_t)a.m >> 32), o);
  r.m = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  return r;
}

// The aggregate of the 8 consecutive items a thread owns, and the inclusive scan of those over the workgroup.  Only
// the list's last workgroup has threads behind the end; what they compute is never used.  Returns the exclusive aggregate of the thread (what
// lies before its first item inside the workgroup; c of the workgroup's first thread is its own first chrom, m
// nothing); *total (thread 255) is the workgroup's aggregate.
__device__ inline RmoAgg rmo_block_scan(int64_t n, const int32_t *chrom, const int64_t *end, int64_t i0, RmoAgg *total) {
  __shared__ RmoAgg wagg[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  RmoAgg mine;
  mine.c = i0 < n ? chrom[i0] : chrom[n - 1];
  mine.m = INT64_MIN;
  for (int q = 0; q < 8; ++q)
    if (i0 + q < n) {
      RmoAgg it;
      it.c = chrom[i0 + q];
      it.m = end[i0 + q];
      mine = rmo_join(mine, it);
    }
  RmoAgg incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const RmoAgg y = rmo_shfl_up(incl, o);
    if (lane >= o) incl = rmo_join(y, incl);
  }
  if (lane == 63) wagg[w] = incl;
  __syncthreads();
  RmoAgg excl = rmo_shfl_up(incl, 1);
  if (lane == 0) {
    excl.c = mine.c;
    excl.m = INT64_MIN;
  }
  RmoAgg before;
  before.c = excl.c;
  before.m = INT64_MIN;
  bool any = false;
  for (int q = 0; q < w; ++q) {
    before = any ? rmo_join(before, wagg[q]) : wagg[q];
    any = true;
  }
  if (any) excl = lane == 0 ? before : rmo_join(before, excl);
  if (total && threadIdx.x == 255) *total = rmo_join(excl, mine);
  return excl;
}

__global__ __launch_bounds__(256) void k_rmo_blockagg(int64_t n, const int32_t *chrom, const int64_t *end,
                                                      int32_t *agg_c, int64_t *agg_m) {
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  RmoAgg tot;
  rmo_block_scan(n, chrom, end, i0, &tot);
  if (threadIdx.x == 255) {
    agg_c[blockIdx.x] = tot.c;
    agg_m[blockIdx.x] = tot.m;
  }
}

// exclusive scan of the workgroup aggregates in place (one workgroup): entry b becomes what lies before block b
__global__ __launch_bounds__(256) void k_rmo_scan_blocks(int64_t n_blocks, int32_t *agg_c, int64_t *agg_m) {
  __shared__ RmoAgg sh[256];
  __shared__ RmoAgg carry_s;
  __shared__ int have_carry;
  if (threadIdx.x == 0) have_carry = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < n_blocks; b0 += 256) {
    const int64_t i = b0 + threadIdx.x;
    const int64_t last = b0 + 255 < n_blocks ? b0 + 255 : n_blocks - 1;
    RmoAgg v;                                              // (threads behind the end repeat the last block: harmless)
    v.c = agg_c[i < n_blocks ? i : last];
    v.m = i < n_blocks ? agg_m[i] : INT64_MIN;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      RmoAgg mine = sh[threadIdx.x];
      if (threadIdx.x >= (unsigned)o) mine = rmo_join(sh[threadIdx.x - o], mine);
      __syncthreads();
      sh[threadIdx.x] = mine;
      __syncthreads();
    }
    RmoAgg excl;
    excl.c = v.c;
    excl.m = INT64_MIN;
    if (threadIdx.x > 0) excl = sh[threadIdx.x - 1];
    if (have_carry) excl = threadIdx.x > 0 ? rmo_join(carry_s, excl) : carry_s;
    const RmoAgg incl = rmo_join(excl, v);
    if (i < n_blocks) {
      agg_c[i] = excl.c;
      agg_m[i] = excl.m;
    }
    __syncthreads();
    if (threadIdx.x == 255) {
      carry_s = incl;
      have_carry = 1;
    }
    __syncthreads();
  }
}

// new_start[i] = max(start[i], every earlier end of the chromosome); keep[i] = end[i] > new_start[i]
__global__ __launch_bounds__(256) void k_rmo_apply(int64_t n, const int32_t *chrom, const int64_t *start,
                                                   const int64_t *end, const int32_t *agg_c, const int64_t *agg_m,
                                                   int64_t *new_start, uint8_t *keep) {
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  RmoAgg p = rmo_block_scan(n, chrom, end, i0, nullptr);
  RmoAgg carry;
  carry.c = agg_c[blockIdx.x];
  carry.m = agg_m[blockIdx.x];
  p = rmo_join(carry, p);
  for (int q = 0; q < 8; ++q) {
    const int64_t i = i0 + q;
    if (i >= n) break;
    RmoAgg it;
    it.c = chrom[i];
    it.m = end[i];
    const int64_t s = start[i];
    const int64_t ns = p.c == it.c && p.m > s ? p.m : s;
    new_start[i] = ns;
    keep[i] = it.m > ns ? 1 : 0;
    p = rmo_join(p, it);
  }
}

// out_index[rank] = i, out_start[rank] = new_start[i] for the kept intervals, up to cap
__global__ __launch_bounds__(256) void k_rmo_scatter(int64_t n, const uint8_t *keep, const unsigned *block_cnt,
                                                     const int64_t *new_start, int64_t cap, int64_t *out_index,
                                                     int64_t *out_start) {
  __shared__ unsigned wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  unsigned c[8], mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = (i0 + q < n && keep[i0 + q] != 0) ? 1u : 0u;
    mine += c[q];
  }
  unsigned incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  int64_t rank = (int64_t)block_cnt[blockIdx.x] + incl - mine;
  for (int q = 0; q < w; ++q) rank += wtot[q];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (!c[q]) continue;
    if (rank < cap) {
      out_index[rank] = i0 + q;
      out_start[rank] = new_start[i0 + q];
    }
    ++rank;
  }
}

}  // namespace tehmm
