// tehmm_masking.hip.h -- interval algebra on the mask tracks outside the HMM: what
// cutOutMaskIntervals (bin/compareBedStates.py:680-710) gets from sortBed | mergeBed | filterBedLengths | subtractBed,
// the intersectBed of bin/interpolateMaskedRegions.py, and that tool's flank loop (lines 117-162).
//
// Lists are (chrom id, start, end) columns; chrom ids follow the byte-wise order of the names, so id order is the
// order of sortBed.  "Sorted": chrom ids never decrease and, inside a chrom, starts never decrease.  "Disjoint":
// sorted, and start[i] >= end[i - 1] inside a chrom.
//
//   k_msk_check                      start < end for every interval, and the order a list must have
//   merge      k_rmo_blockagg, k_rmo_scan_blocks (the running maximum of tehmm_tsd.hip.h), k_msk_merge_apply: run
//              heads and the inclusive running maximum; k_msk_merge_runs: one row per run; k_msk_len_flags and
//              k_msk_compact: the length filter
//   subtract / intersect
//              k_msk_count: pieces of every a from two binary searches into B (subtract: plus the two end pieces and
//              the gaps between its b, a difference of the scanned gap flags of B); a 64-bit exclusive scan over A;
//              k_msk_emit: ONE LANE PER OUTPUT PIECE -- the lane finds its a by a search in the scanned counts and its
//              piece from the two b beside it.  No lane walks B: an interval that spans a million masks costs its
//              lanes what any other piece costs.
//   fill       k_msk_fill: one lane per mask, a lower bound into the prediction and the reference's state choice
#pragma once
#include "tehmm_tsd.hip.h"

namespace tehmm {

#define TEHMM_MASK_MAX_LABELS 2048
#define TEHMM_MASK_ORDER_NONE 0         // any order
#define TEHMM_MASK_ORDER_SORTED 1       // (chrom, start)
#define TEHMM_MASK_ORDER_DISJOINT 2     // sorted, and no interval starts before its predecessor ends
#define TEHMM_MASK_ORDER_TRIPLE 3       // (chrom, start, end)

struct MskView {
  int64_t n;
  const int32_t *chrom;
  const int64_t *start, *end;
};

// viol[0] (preset to ~0): lowest i with start >= end; viol[1]: lowest i that breaks the order against i - 1
__global__ __launch_bounds__(256) void k_msk_check(MskView v, int order, unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < v.n; i += step) {
    const int64_t s = v.start[i], e = v.end[i];
    if (s >= e) atomicMin(viol, (unsigned long long)i);
    if (order == TEHMM_MASK_ORDER_NONE || i == 0) continue;
    const int32_t c = v.chrom[i], cp = v.chrom[i - 1];
    bool bad = c < cp;
    if (c == cp) {
      const int64_t sp = v.start[i - 1], ep = v.end[i - 1];
      bad = s < sp || (order == TEHMM_MASK_ORDER_DISJOINT && s < ep) ||
            (order == TEHMM_MASK_ORDER_TRIPLE && s == sp && e < ep);
    }
    if (bad) atomicMin(viol + 1, (unsigned long long)i);
  }
}

// viol (preset to ~0): lowest i with a label outside [0, L)
__global__ __launch_bounds__(256) void k_msk_labels(int64_t n, const int32_t *label, int L, unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
    if (label[i] < 0 || label[i] >= L) atomicMin(viol, (unsigned long long)i);
}

// ---- exclusive scan of unsigned counts with 64-bit sums (a count is at most 2^31: a workgroup's sum needs them) -------
__device__ inline int64_t msk_shfl_up64(int64_t v, int o) {
  const int lo = __shfl_up((int)(uint32_t)(uint64_t)v, o), hi = __shfl_up((int)((uint64_t)v >> 32), o);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// exclusive prefix of `mine` over the workgroup's threads; *total (valid in every thread) the workgroup's sum
__device__ inline int64_t msk_block_excl(int64_t mine, int64_t *total) {
  __shared__ int64_t wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = msk_shfl_up64(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  int64_t before = incl - mine;
  for (int q = 0; q < w; ++q) before += wtot[q];
  if (total) *total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  return before;
}

__global__ __launch_bounds__(256) void k_msk_blocksum(int64_t n, const uint32_t *count, int64_t *block_sum) {
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  int64_t mine = 0, total;
  for (int q = 0; q < 8; ++q)
    if (i0 + q < n) mine += (int64_t)count[i0 + q];
  msk_block_excl(mine, &total);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// off[i] = sum of count[0 .. i); block_sum after k_tsd_scan_blocks
__global__ __launch_bounds__(256) void k_msk_offsets(int64_t n, const uint32_t *count, const int64_t *block_sum,
                                                     int64_t *off) {
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  uint32_t c[8];
  int64_t mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = i0 + q < n ? count[i0 + q] : 0u;
    mine += (int64_t)c[q];
  }
  int64_t before = block_sum[blockIdx.x] + msk_block_excl(mine, nullptr);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (i0 + q < n) off[i0 + q] = before;
    before += (int64_t)c[q];
  }
}

// ---- merge --------------------------------------------------------------------------------------------------------
// head[i] = 1 when interval i opens a run: nothing of its chrom lies before it, or every earlier end of the chrom is
// below its start (abutting continues the run, as mergeBed does); rmax[i] = maximum of the chrom's ends up to and
// including i.  Every end before a run's head is below the head's start, so at the last interval of a run rmax is
// the run's end.
__global__ __launch_bounds__(256) void k_msk_merge_apply(int64_t n, const int32_t *chrom, const int64_t *start,
                                                         const int64_t *end, const int32_t *agg_c, const int64_t *agg_m,
                                                         uint8_t *head, int64_t *rmax) {
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
    const bool cont = p.c == it.c && p.m != INT64_MIN && p.m >= start[i];
    head[i] = cont ? 0 : 1;
    p = rmo_join(p, it);
    rmax[i] = p.m;
  }
}

// run r = heads before its head: (chrom, start) of the head, end = rmax of the run's last interval (the one before the
// next head, or the list's last); block_cnt: the scanned head counts of k_seg_count
__global__ __launch_bounds__(256) void k_msk_merge_runs(int64_t n, const uint8_t *head, const unsigned *block_cnt,
                                                        const int32_t *chrom, const int64_t *start, const int64_t *rmax,
                                                        int32_t *run_c, int64_t *run_s, int64_t *run_e) {
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  unsigned c[8];
  int64_t mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = (i0 + q < n && head[i0 + q] != 0) ? 1u : 0u;
    mine += c[q];
  }
  int64_t rank = (int64_t)block_cnt[blockIdx.x] + msk_block_excl(mine, nullptr);      // heads before i0
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t i = i0 + q;
    if (i >= n) break;
    if (c[q]) {
      run_c[rank] = chrom[i];
      run_s[rank] = start[i];
      ++rank;
    }
    const bool tail = i + 1 == n || (q < 7 ? c[q + 1] != 0 : head[i + 1] != 0);
    if (tail) run_e[rank - 1] = rmax[i];
  }
}

// keep[r] = min_len <= end - start <= max_len (end > start: the difference fits 64 unsigned bits)
__global__ __launch_bounds__(256) void k_msk_len_flags(int64_t n, const int64_t *s, const int64_t *e, int64_t min_len,
                                                       int64_t max_len, uint8_t *keep) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    const uint64_t len = (uint64_t)e[i] - (uint64_t)s[i];
    keep[i] = max_len >= 0 && len <= (uint64_t)max_len && (min_len <= 0 || len >= (uint64_t)min_len) ? 1 : 0;
  }
}

// the kept rows in order, up to cap; block_cnt: the scanned keep counts of k_seg_count
__global__ __launch_bounds__(256) void k_msk_compact(int64_t n, const uint8_t *keep, const unsigned *block_cnt,
                                                     const int32_t *c_in, const int64_t *s_in, const int64_t *e_in,
                                                     int64_t cap, int32_t *c_out, int64_t *s_out, int64_t *e_out) {
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  unsigned c[8];
  int64_t mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = (i0 + q < n && keep[i0 + q] != 0) ? 1u : 0u;
    mine += c[q];
  }
  int64_t rank = (int64_t)block_cnt[blockIdx.x] + msk_block_excl(mine, nullptr);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (!c[q]) continue;
    if (rank < cap) {
      c_out[rank] = c_in[i0 + q];
      s_out[rank] = s_in[i0 + q];
      e_out[rank] = e_in[i0 + q];
    }
    ++rank;
  }
}

// ---- subtract and intersect -------------------------------------------------------------------------------------------
// gap[j] = 1 when a gap lies between b[j - 1] and b[j] (same chrom, start[j] > end[j - 1]); gap[0] = gap[nB] = 0.
// Its exclusive scan G [nB + 1] counts the gaps inside any range of B in constant time, abutting b included.
__global__ __launch_bounds__(256) void k_msk_gap_flags(MskView b, uint32_t *gap) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= b.n; j += step)
    gap[j] = j > 0 && j < b.n && b.chrom[j] == b.chrom[j - 1] && b.start[j] > b.end[j - 1] ? 1u : 0u;
}

// first j with (chrom, end) of b[j] above (c, x): the first b of chrom c that ends behind x, or the first b of a
// later chrom.  B is disjoint, so inside a chrom ends ascend with starts.
__device__ inline int64_t msk_first_end_above(const MskView &b, int32_t c, int64_t x) {
  int64_t lo = 0, hi = b.n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int32_t cm = b.chrom[mid];
    if (cm > c || (cm == c && b.end[mid] > x)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// first j with (chrom, start) of b[j] at or above (c, x)
__device__ inline int64_t msk_first_start_from(const MskView &b, int32_t c, int64_t x) {
  int64_t lo = 0, hi = b.n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int32_t cm = b.chrom[mid];
    if (cm > c || (cm == c && b.start[mid] >= x)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The b that overlap a are b[lo .. hi).  intersect: hi - lo pieces.  subtract: the part of a before b[lo], the gaps
// between lo and hi - 1, the part behind b[hi - 1]; a itself when no b overlaps it.
template <bool SUB>
__global__ __launch_bounds__(256) void k_msk_count(MskView a, MskView b, const int64_t *G, uint32_t *count, int32_t *lo_out,
                                                   int32_t *hi_out) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += step) {
    const int32_t c = a.chrom[i];
    const int64_t s = a.start[i], e = a.end[i];
    const int64_t lo = msk_first_end_above(b, c, s), hi = msk_first_start_from(b, c, e);
    uint32_t cnt = (uint32_t)(hi - lo);
    if (SUB) {
      if (hi == lo) cnt = 1;
      else
        cnt = (b.start[lo] > s ? 1u : 0u) + (uint32_t)(G[hi] - G[lo + 1]) + (b.end[hi - 1] < e ? 1u : 0u);
    }
    count[i] = cnt;
    lo_out[i] = (int32_t)lo;
    hi_out[i] = (int32_t)hi;
  }
}

// piece r belongs to the last a with off[a] <= r (an a without pieces shares its offset with its successor)
__device__ inline int64_t msk_owner(int64_t n, const int64_t *off, int64_t r) {
  int64_t lo = 0, hi = n;      // first index with off > r
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] > r) hi = mid;
    else lo = mid + 1;
  }
  return lo - 1;
}

template <bool SUB>
__global__ __launch_bounds__(256) void k_msk_emit(int64_t n_write, MskView a, MskView b, const int64_t *G,
                                                  const int64_t *off, const int32_t *lo_in, const int32_t *hi_in,
                                                  int64_t *out_src, int64_t *out_start, int64_t *out_end) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_write; r += step) {
    const int64_t i = msk_owner(a.n, off, r);
    int64_t p = r - off[i];
    const int64_t s = a.start[i], e = a.end[i], lo = lo_in[i], hi = hi_in[i];
    int64_t ps, pe;
    if (!SUB) {
      const int64_t bs = b.start[lo + p], be = b.end[lo + p];
      ps = bs > s ? bs : s;
      pe = be < e ? be : e;
    } else if (hi == lo) {
      ps = s;
      pe = e;
    } else {
      const bool first = b.start[lo] > s;
      const int64_t inner = G[hi] - G[lo + 1];
      if (first && p == 0) {
        ps = s;
        pe = b.start[lo];
      } else {
        p -= first ? 1 : 0;
        if (p < inner) {
          // the (p + 1)-th gap flag behind lo: the first j in (lo, hi) with G[j + 1] >= G[lo + 1] + p + 1
          const int64_t want = G[lo + 1] + p + 1;
          int64_t x = lo + 1, y = hi - 1;
          while (x < y) {
            const int64_t mid = x + ((y - x) >> 1);
            if (G[mid + 1] >= want) y = mid;
            else x = mid + 1;
          }
          ps = b.end[x - 1];
          pe = b.start[x];
        } else {
          ps = b.end[hi - 1];
          pe = e;
        }
      }
    }
    out_src[r] = i;
    out_start[r] = ps;
    out_end[r] = pe;
  }
}

// ---- the flank loop of interpolateMaskedRegions.py:117-162 ---------------------------------------------------------
struct MskFill {
  MskView m, iv;
  const int32_t *label;
  const uint8_t *two, *one;      // [L] flags
  int only_default;
  int64_t max_len;
};

// out[x]: -2 for a mask longer than max_len (not filled), -1 for the default, else the label; viol (preset to ~0):
// lowest mask with a candidate flank of its chrom that overlaps it without abutting
__global__ __launch_bounds__(256) void k_msk_fill(MskFill f, int32_t *out, unsigned long long *viol) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < f.m.n; x += step) {
    const int32_t c = f.m.chrom[x];
    const int64_t s = f.m.start[x], e = f.m.end[x];
    if ((uint64_t)e - (uint64_t)s > (uint64_t)(f.max_len < 0 ? 0 : f.max_len)) {
      out[x] = -2;
      continue;
    }
    // where the reference's pointer stands: the first interval whose (chrom, start, end) is not below the mask's
    int64_t lo = 0, hi = f.iv.n;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      const int32_t cm = f.iv.chrom[mid];
      const int64_t sm = f.iv.start[mid];
      const bool ge = cm > c || (cm == c && (sm > s || (sm == s && f.iv.end[mid] >= e)));
      if (ge) hi = mid;
      else lo = mid + 1;
    }
    // behind the last interval the pointer has stopped ON the last index and the right flank is gone
    const int64_t right = lo < f.iv.n ? lo : -1;
    const int64_t left = lo < f.iv.n ? lo - 1 : f.iv.n - 2;
    int32_t ls = -1, rs = -1;
    bool clash = false;
    if (left >= 0 && f.iv.chrom[left] == c) {
      const int64_t a = f.iv.start[left], b = f.iv.end[left];
      if (b == s) ls = f.label[left];
      else clash = (b < e ? b : e) > (a > s ? a : s);
    }
    if (right >= 0 && f.iv.chrom[right] == c) {
      const int64_t a = f.iv.start[right], b = f.iv.end[right];
      if (a == e) rs = f.label[right];
      else clash = clash || (b < e ? b : e) > (a > s ? a : s);
    }
    if (clash) atomicMin(viol, (unsigned long long)x);
    int32_t state = -1;
    if (f.only_default) state = -1;
    else if (ls >= 0 && ls == rs) state = f.two[ls] ? ls : -1;
    else if (ls >= 0 && f.one[ls]) state = ls;
    else if (rs >= 0 && f.one[rs]) state = rs;
    out[x] = state;
  }
}

}  // namespace tehmm
