// tehmm_compare.hip.h -- comparison of two state annotations (bin/compareBedStates.py, bin/fitStateNames.py) as device
// kernels on interval lists.
//
// An interval list is n rows (chrom id, start, end, label), sorted, without self-overlap; two lists of a comparison
// cover the same bases.  Nothing here walks the two lists side by side: every work item finds its place in the other
// list by one binary search on (chrom, start).
//
//   validity and cover      k_cmp_valid, k_cmp_cover       lowest offending index per list, by atomicMin
//   base-level confusion    k_cmp_base                     one item per interval of EITHER list: the piece it owns
//   one-sided intervals     k_cmp_intervals / _long        one item per true interval; long pred ranges one wave each
//   run merge               k_mrg_flags / _scatter         head flags, k_seg_count + k_scan_blocks, scatter
//
// All counts are 64-bit integers added with atomics (LDS matrices per workgroup up to TEHMM_CMP_LDS_LABELS labels,
// the global matrix above), so no result depends on an order.  The one order-bound number, the running sum of
// fractions of a true interval, is taken by one lane or one wave in list order.  No kernel waits on another workgroup.
#pragma once
#include "tehmm_segment.hip.h"

namespace tehmm {

#define TEHMM_CMP_MAX_LABELS 2048
#define TEHMM_CMP_LDS_LABELS 64       // [64][64] cells + 4 x 64 counters of 8 bytes: 34 KB of LDS per workgroup
#define TEHMM_CMP_LONG_RANGE 128      // pred ranges longer than this go to k_cmp_intervals_long

struct CmpList {
  int64_t n;
  const int32_t *chrom;
  const int64_t *start;
  const int64_t *end;
  const int32_t *label;
};

// the last interval of y with (chrom, start) <= (c, p), or -1; the result is always inside [-1, n)
__device__ inline int64_t cmp_find(const CmpList &y, int32_t c, int64_t p) {
  int64_t lo = -1, hi = y.n;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int32_t cm = y.chrom[mid];
    if (cm < c || (cm == c && y.start[mid] <= p)) lo = mid;
    else hi = mid;
  }
  return lo;
}

// viol[0], viol[1] (preset to ~0): lowest index of list 1 / list 2 that is empty, carries a label outside [0, L),
// lies on a lower chrom than its predecessor or starts inside it
__global__ __launch_bounds__(256) void k_cmp_valid(CmpList a, CmpList b, int L, unsigned long long *viol) {
  const int64_t n = a.n + b.n, step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += step) {
    const bool first = x < a.n;
    const CmpList &l = first ? a : b;
    const int64_t i = first ? x : x - a.n;
    const int32_t c = l.chrom[i], lab = l.label[i];
    const int64_t s = l.start[i];
    bool bad = !(s < l.end[i]) || lab < 0 || lab >= L;
    if (i > 0) {
      const int32_t cp = l.chrom[i - 1];
      bad = bad || c < cp || (c == cp && s < l.end[i - 1]);
    }
    if (bad) atomicMin(&viol[first ? 0 : 1], (unsigned long long)i);
  }
}

// Equal cover of two VALID lists without a walk: every region start of x (an interval no predecessor abuts) must be a
// region start of y at the same base, every region end a region end; viol[0] / viol[1] (preset to ~0) get the lowest
// index of list 1 / list 2 with a boundary that is none in the other list.
__global__ __launch_bounds__(256) void k_cmp_cover(CmpList a, CmpList b, unsigned long long *viol) {
  const int64_t n = a.n + b.n, step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += step) {
    const bool first = x < a.n;
    const CmpList &X = first ? a : b, &Y = first ? b : a;
    const int64_t i = first ? x : x - a.n;
    const int32_t c = X.chrom[i];
    const int64_t s = X.start[i], e = X.end[i];
    const bool rs = i == 0 || X.chrom[i - 1] != c || X.end[i - 1] != s;
    const bool re = i == X.n - 1 || X.chrom[i + 1] != c || X.start[i + 1] != e;
    bool bad = false;
    if (rs) {      // base s lies in y's cover and base s - 1 does not
      const int64_t j = cmp_find(Y, c, s);
      bad = j < 0 || Y.chrom[j] != c || Y.start[j] != s || (j > 0 && Y.chrom[j - 1] == c && Y.end[j - 1] == s);
    }
    if (re && !bad) {      // base e - 1 lies in y's cover and base e does not
      const int64_t j = cmp_find(Y, c, e - 1);
      bad = j < 0 || Y.chrom[j] != c || Y.end[j] != e || (j + 1 < Y.n && Y.chrom[j + 1] == c && Y.start[j + 1] == e);
    }
    if (bad) atomicMin(&viol[first ? 0 : 1], (unsigned long long)i);
  }
}

// ---- accumulation: a workgroup's LDS copy of the cells, flushed once, or the global cells directly ------------------
template <bool LDS>
__device__ inline unsigned long long *cmp_acc_begin(unsigned long long *lds, unsigned long long *glob, int cells) {
  if (!LDS) return glob;
  for (int x = threadIdx.x; x < cells; x += 256) lds[x] = 0;
  __syncthreads();
  return lds;
}

template <bool LDS>
__device__ inline void cmp_acc_end(unsigned long long *lds, unsigned long long *glob, int cells) {
  if (!LDS) return;
  __syncthreads();
  for (int x = threadIdx.x; x < cells; x += 256) {
    const unsigned long long v = lds[x];
    if (v) atomicAdd(&glob[x], v);
  }
}

// first[cell] (NULL: not wanted; preset to ~0) = the lowest (index in the walked list << 32 | index in the other list)
// at which the cell was added to: the place where the reference's walk inserts the pair into its dict.  Always global.
// The read in front only spares atomics -- a stale, higher value costs one more atomicMin, never a wrong result -- and
// is an agent-scope load, served by L2: a line kept in a CU's L1 would stay at ~0 for the whole kernel.
__device__ inline void cmp_note_first(unsigned long long *first, int cell, int64_t walked, int64_t other) {
  if (!first) return;
  const unsigned long long key = ((unsigned long long)walked << 32) | (unsigned long long)other;
  if (key < __hip_atomic_load(&first[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&first[cell], key);
}

// Base level.  Every maximal piece on which both lists keep one interval each begins at the start of exactly one
// interval (of list 1 where both start there): the item of that interval adds the piece's length to
// conf[label 1][label 2].  One search and one add per item, whatever the lengths.
template <bool LDS>
__global__ __launch_bounds__(256) void k_cmp_base(CmpList a, CmpList b, int L, unsigned long long *conf,
                                                  unsigned long long *first_seen) {
  extern __shared__ unsigned long long cmp_lds[];
  unsigned long long *acc = cmp_acc_begin<LDS>(cmp_lds, conf, L * L);
  const int64_t n = a.n + b.n, step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += step) {
    const bool first = x < a.n;
    const CmpList &X = first ? a : b, &Y = first ? b : a;
    const int64_t i = first ? x : x - a.n;
    const int32_t c = X.chrom[i];
    const int64_t s = X.start[i], e = X.end[i];
    const int64_t j = cmp_find(Y, c, s);
    if (j < 0 || Y.chrom[j] != c) continue;              // (cannot happen on checked lists)
    const int64_t ye = Y.end[j];
    if (ye <= s || (!first && Y.start[j] == s)) continue;      // list 1 owns a piece both lists start
    const int64_t len = (e < ye ? e : ye) - s;
    const int32_t lx = X.label[i], ly = Y.label[j];
    const int cell = first ? lx * L + ly : ly * L + lx;
    atomicAdd(&acc[cell], (unsigned long long)len);
    cmp_note_first(first_seen, cell, first ? i : j, first ? j : i);
  }
  cmp_acc_end<LDS>(cmp_lds, conf, L * L);
}

// cells of the one-sided pass: conf [L][L], then n_hit, len_hit, n_miss, len_miss [L] each
__host__ __device__ inline int cmp_interval_cells(int L) { return L * L + 4 * L; }

struct CmpIntervalOpt {
  int L;
  double threshold;
  int use_pred_len;
  int allow_multiple;
};

// the preds overlapping true interval i: [j0, j1], empty (j1 < j0) only on lists that were not checked
__device__ inline void cmp_pred_range(const CmpList &t, const CmpList &p, int64_t i, int64_t &j0, int64_t &j1) {
  const int32_t c = t.chrom[i];
  j0 = cmp_find(p, c, t.start[i]);
  j1 = cmp_find(p, c, t.end[i] - 1);
  if (j0 < 0 || p.chrom[j0] != c || p.end[j0] <= t.start[i]) ++j0;
}

// overlap fraction of pred j against true interval [s, e): IEEE division of the two converted integers
__device__ inline double cmp_fraction(const CmpList &p, int64_t j, int64_t s, int64_t e, int use_pred_len) {
  const int64_t ps = p.start[j], pe = p.end[j];
  const int64_t ov = (pe < e ? pe : e) - (ps > s ? ps : s);
  return (double)ov / (double)(use_pred_len ? pe - ps : e - s);
}

__device__ inline void cmp_interval_result(unsigned long long *acc, const CmpIntervalOpt &o, int32_t lab, int64_t len,
                                           double best, double total) {
  const bool hit = (o.allow_multiple ? total : best) >= o.threshold;
  unsigned long long *st = acc + o.L * o.L + (hit ? 0 : 2 * o.L);
  atomicAdd(&st[lab], 1ull);
  atomicAdd(&st[o.L + lab], (unsigned long long)len);
}

// One item per true interval: the walk over its preds in list order.  An interval with more than
// TEHMM_CMP_LONG_RANGE preds is not walked here: its index goes to long_idx[] (any order) for k_cmp_intervals_long.
template <bool LDS>
__global__ __launch_bounds__(256) void k_cmp_intervals(CmpList t, CmpList p, CmpIntervalOpt o, unsigned long long *out,
                                                       unsigned long long *first_seen, int32_t *long_idx,
                                                       unsigned long long *n_long) {
  extern __shared__ unsigned long long cmp_lds[];
  const int cells = cmp_interval_cells(o.L);
  unsigned long long *acc = cmp_acc_begin<LDS>(cmp_lds, out, cells);
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += step) {
    int64_t j0, j1;
    cmp_pred_range(t, p, i, j0, j1);
    if (j1 - j0 >= TEHMM_CMP_LONG_RANGE) {
      long_idx[atomicAdd(n_long, 1ull)] = (int32_t)i;      // at most one entry per i: never beyond t.n
      continue;
    }
    const int64_t s = t.start[i], e = t.end[i];
    const int32_t lab = t.label[i];
    double best = 0.0, total = 0.0;
    for (int64_t j = j0; j <= j1; ++j) {
      const double frac = cmp_fraction(p, j, s, e, o.use_pred_len);
      const int32_t pl = p.label[j];
      if (pl == lab) {
        best = frac > best ? frac : best;
        total += frac;
      }
      if (frac >= o.threshold) {
        atomicAdd(&acc[pl * o.L + lab], 1ull);
        cmp_note_first(first_seen, pl * o.L + lab, i, j);
      }
    }
    cmp_interval_result(acc, o, lab, e - s, best, total);
  }
  cmp_acc_end<LDS>(cmp_lds, out, cells);
}

// One wave per long true interval: the lanes fetch 64 preds and divide; the fractions of equal label are then taken
// through lane after lane, in list order, into the running sum (every lane keeps the same sum).
template <bool LDS>
__global__ __launch_bounds__(256) void k_cmp_intervals_long(CmpList t, CmpList p, CmpIntervalOpt o,
                                                            unsigned long long *out,
                                                            unsigned long long *first_seen, const int32_t *long_idx,
                                                            int64_t n_long) {
  extern __shared__ unsigned long long cmp_lds[];
  const int cells = cmp_interval_cells(o.L);
  unsigned long long *acc = cmp_acc_begin<LDS>(cmp_lds, out, cells);
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_long; w += step) {
    const int64_t i = long_idx[w];
    int64_t j0, j1;
    cmp_pred_range(t, p, i, j0, j1);
    const int64_t s = t.start[i], e = t.end[i];
    const int32_t lab = t.label[i];
    double best = 0.0, total = 0.0;
    for (int64_t base = j0; base <= j1; base += 64) {
      const int64_t j = base + lane;
      double frac = 0.0;
      bool same = false;
      if (j <= j1) {
        frac = cmp_fraction(p, j, s, e, o.use_pred_len);
        const int32_t pl = p.label[j];
        same = pl == lab;
        if (frac >= o.threshold) {
          atomicAdd(&acc[pl * o.L + lab], 1ull);
          cmp_note_first(first_seen, pl * o.L + lab, i, j);
        }
      }
      unsigned long long m = __ballot(same);
      while (m) {
        const double f = __shfl(frac, (int)__builtin_ctzll(m));
        best = f > best ? f : best;
        total += f;
        m &= m - 1;
      }
    }
    if (lane == 0) cmp_interval_result(acc, o, lab, e - s, best, total);
  }
  cmp_acc_end<LDS>(cmp_lds, out, cells);
}

// ---- run merge (fitStateNames.py writeFittedBed) -------------------------------------------------------------------
// mapped[i] = lut ? lut[label[i]] : label[i]; head[i] = 1 unless interval i continues the run of i - 1 (same chrom,
// same mapped label, start[i] == end[i - 1]).  A label outside [0, L) is never looked up: *viol (preset to ~0) gets
// the lowest such index and the caller gives up.
__device__ inline int32_t mrg_map(const int32_t *lut, int L, int32_t lab) {
  return lut && lab >= 0 && lab < L ? lut[lab] : lab;
}

__global__ __launch_bounds__(256) void k_mrg_flags(CmpList l, int L, const int32_t *lut, int32_t *mapped, uint8_t *head,
                                                   unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < l.n; i += step) {
    const int32_t lab = l.label[i];
    if (lab < 0 || lab >= L) atomicMin(viol, (unsigned long long)i);
    const int32_t m = mrg_map(lut, L, lab);
    bool h = true;
    if (i > 0) h = mrg_map(lut, L, l.label[i - 1]) != m || l.chrom[i - 1] != l.chrom[i] || l.end[i - 1] != l.start[i];
    mapped[i] = m;
    head[i] = h ? 1 : 0;
  }
}

// rank of a run = number of heads before its head (block_cnt: exclusive scan of the per-block head counts); the head
// writes chrom, start and label of the run, its last interval the end
__global__ __launch_bounds__(256) void k_mrg_scatter(CmpList l, const int32_t *mapped, const uint8_t *head,
                                                     const unsigned *block_cnt, int32_t *out_chrom, int64_t *out_start,
                                                     int64_t *out_end, int32_t *out_label) {
  __shared__ unsigned wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  unsigned c[8], mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = (i0 + q < l.n && head[i0 + q] != 0) ? 1u : 0u;
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
  int64_t heads = (int64_t)block_cnt[blockIdx.x] + incl - mine;      // heads before i0
  for (int q = 0; q < w; ++q) heads += wtot[q];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t i = i0 + q;
    if (i >= l.n) break;
    if (c[q]) {
      out_chrom[heads] = l.chrom[i];
      out_start[heads] = l.start[i];
      out_label[heads] = mapped[i];
      ++heads;
    }
    if (i + 1 == l.n || head[i + 1] != 0) out_end[heads - 1] = l.end[i];      // heads >= 1: interval 0 is a head
  }
}

}  // namespace tehmm
