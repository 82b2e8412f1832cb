// tehmm_segment.hip.h -- track segmentation (bin/segmentTracks.py:200-277) as device kernels: the cut rows of
// unsegmented uint8 track tables.
//
// The reference walks one chain per table: row i opens a new segment when it differs from the reference row of the
// running segment in a cut track or in more than `thresh` tracks, or when the segment has reached maxLen rows.  The
// whole state of that chain before row i is ONE number, the row L of the last cut (the table's first row counts as
// one): the running length is i - L, the reference row is L (--comp first) or i - 1 (--comp prev).
//
//   fixLen > 0                      closed form, no data                               k_seg_fixlen
//   comp = prev, maxLen == 0        every decision reads rows i, i - 1 only            k_seg_prev_flags
//   otherwise                       speculate per stripe, link, re-walk what is left   k_seg_spec / _link / _rewalk
//
// Rows are packed to dwords first (ignored tracks zeroed, row padded with zeros to a multiple of four bytes), so
// "number of differing tracks" is a popcount over xor-ed dwords and "a cut track differs" is one AND with a mask.
// A wave holds 64 consecutive rows, one per lane: the 64 rows are one contiguous block of memory.
#pragma once
#include "tehmm_aux.hip.h"

namespace tehmm {

#define TEHMM_SEG_STRIPE 1024      // rows per stripe of the speculative pass

// data [total][K] bytes -> packed [total][KW] dwords
__global__ __launch_bounds__(256) void k_seg_pack(int64_t total, int K, int KW, const uint8_t *data,
                                                  const uint8_t *ignore, uint32_t *packed) {
  const int64_t n = total * KW, step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += step) {
    const int64_t row = x / KW;
    const int w = (int)(x - row * KW);
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = 4 * w + q;
      if (k < K && ignore[k] == 0) v |= (uint32_t)data[row * K + k] << (8 * q);
    }
    packed[x] = v;
  }
}

// number of non-zero bytes of x
__device__ inline int seg_nz_bytes(uint32_t x) {
  return __popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
}

// the data rule of isNewSegment (segmentTracks.py:252-266) for row i against reference row r
__device__ inline bool seg_rule(const uint32_t *packed, int KW, const uint32_t *cutw, int thresh, int64_t i,
                                int64_t r) {
  const uint32_t *a = packed + i * KW, *b = packed + r * KW;
  int dif = 0;
  uint32_t hit = 0;
  for (int w = 0; w < KW; ++w) {
    const uint32_t x = a[w] ^ b[w];
    hit |= x & cutw[w];
    dif += seg_nz_bytes(x);
  }
  return hit != 0 || dif > thresh;
}

struct SegParams {
  const uint32_t *packed;      // [total][KW]
  const uint32_t *cutw;        // [KW], 0xff in the bytes of cut tracks
  int KW;
  int thresh;
  int64_t maxLen;              // 0: none
};

// One wave walks rows [from, end) of a table from the state "last cut at row L" (L < from, L + maxLen >= from).
// on_cut(c) is called, wave-uniformly and in ascending order, for every row the chain cuts at; it returns true to
// end the walk.  Returns true when on_cut ended the walk; L is the last cut either way.
// 64 rows are decided per step: the lanes evaluate the data rule, __ballot and a count of trailing zeros give the
// first data cut, and maxLen folds in as min(first data cut, L + maxLen).  In first mode the reference row changes
// with every cut, so the step after a cut starts at the row behind it; in prev mode the 64 decisions stand and the
// remaining bits of the ballot are consumed.
template <bool PREV, class OnCut>
__device__ inline bool seg_walk(const SegParams &p, int64_t &L, int64_t from, int64_t end, int lane, OnCut on_cut) {
  int64_t base = from;
  while (base < end) {
    const int64_t i = base + lane;
    const bool f = i < end && seg_rule(p.packed, p.KW, p.cutw, p.thresh, i, PREV ? i - 1 : L);
    const unsigned long long mask = __ballot(f);
    const int64_t chunk_end = base + 64 < end ? base + 64 : end;
    int64_t lo = base;                                   // first row of the chunk not decided yet
    for (;;) {
      const unsigned long long m = mask & (~0ull << (int)(lo - base));
      const int64_t first = m ? base + (int64_t)__builtin_ctzll(m) : chunk_end;
      const int64_t lim = p.maxLen > 0 ? L + p.maxLen : chunk_end;
      int64_t c = first < lim ? first : lim;
      if (c < lo) c = lo;                                // (a state with L + maxLen < from: never loop in place)
      if (c >= chunk_end) {
        base = chunk_end;
        break;
      }
      L = c;
      if (on_cut(c)) return true;
      if (!PREV) {
        base = c + 1;
        break;
      }
      lo = c + 1;
      if (lo >= chunk_end) {
        base = chunk_end;
        break;
      }
    }
  }
  return false;
}

// Stripe s covers rows [st_begin[s], st_begin[s + 1]) of the concatenated tables; a stripe never crosses a table
// boundary.  Speculation: every stripe assumes a cut at its first row.  spec[] (zeroed by the caller) gets a 1 at
// every cut behind the first row; spec_exit[s] is the last cut of the speculative chain.
template <bool PREV>
__global__ __launch_bounds__(256) void k_seg_spec(SegParams p, int64_t n_stripes, const int64_t *st_begin,
                                                  uint8_t *spec, int64_t *spec_exit) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_stripes) return;
  const int64_t a = st_begin[s], b = st_begin[s + 1];
  int64_t L = a;
  seg_walk<PREV>(p, L, a + 1, b, lane, [&](int64_t c) {
    if (lane == 0) spec[c] = 1;
    return false;
  });
  if (lane == 0) spec_exit[s] = L;
}

// Link: stripe s (not the first of its table) starts from the speculative exit of stripe s - 1 and walks from its
// own first row until it cuts at a row where its own speculation cut too (its assumed first-row cut included):
// from there on both chains are in the state "last cut = that row" and the speculative flags stand.  Its own
// decisions before that row go to lnk[] (zeroed by the caller); meet[s] is the row where the chains met, or the
// stripe's end when they never did (a marked stripe; link_exit[s] is then the last cut of the walked chain).
// meet[s] of a table's first stripe is its first row: nothing to link.
template <bool PREV>
__global__ __launch_bounds__(256) void k_seg_link(SegParams p, int64_t n_stripes, const int64_t *st_begin,
                                                  const uint8_t *st_first, const uint8_t *spec,
                                                  const int64_t *spec_exit, uint8_t *lnk, int64_t *meet,
                                                  int64_t *link_exit, unsigned long long *n_marked) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_stripes) return;
  const int64_t a = st_begin[s], b = st_begin[s + 1];
  if (st_first[s]) {
    if (lane == 0) meet[s] = a;
    return;
  }
  int64_t L = spec_exit[s - 1];
  int64_t met = b;
  const bool stopped = seg_walk<PREV>(p, L, a, b, lane, [&](int64_t c) {
    if (c == a || spec[c] != 0) {
      met = c;
      return true;
    }
    if (lane == 0) lnk[c] = 1;
    return false;
  });
  if (lane == 0) {
    meet[s] = met;
    if (!stopped) {
      link_exit[s] = L;
      atomicAdd(n_marked, 1ull);
    }
  }
}

// Exact sequential walk of what the link pass could not settle: one wave per table goes through the table's
// stripes in order.  While the speculative exit of the previous stripe is the truth, a stripe's link stands; a marked
// stripe ends that (its own walk started from the truth, so link_exit is the truth), and every stripe after it is
// walked again from the true state until one meets its speculation.  counters[0] += marked or re-walked stripes.
template <bool PREV>
__global__ __launch_bounds__(256) void k_seg_rewalk(SegParams p, int64_t n_tables, const int64_t *tbl_stripe0,
                                                    const int64_t *st_begin, const uint8_t *spec, uint8_t *lnk,
                                                    int64_t *meet, const int64_t *link_exit,
                                                    unsigned long long *counters) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tables) return;
  const int64_t s0 = tbl_stripe0[t], s1 = tbl_stripe0[t + 1];
  unsigned long long touched = 0;
  int64_t s = s0 + 1;
  while (s < s1) {
    // the truth is known at the start of stripe s: find the next marked stripe, 64 at a time
    const int64_t q = s + lane;
    const bool marked = q < s1 && meet[q] == st_begin[q + 1];
    const unsigned long long mk = __ballot(marked);
    if (mk == 0) {
      s += 64;
      continue;
    }
    s += (int64_t)__builtin_ctzll(mk);
    int64_t L = link_exit[s];
    ++touched;
    for (++s; s < s1; ++s) {
      const int64_t a = st_begin[s], b = st_begin[s + 1];
      for (int64_t i = a + lane; i < b; i += 64) lnk[i] = 0;
      __threadfence();                                   // the zeros land before this wave's ones
      int64_t met = b;
      const bool stopped = seg_walk<PREV>(p, L, a, b, lane, [&](int64_t c) {
        if (c == a || spec[c] != 0) {
          met = c;
          return true;
        }
        if (lane == 0) lnk[c] = 1;
        return false;
      });
      if (lane == 0) meet[s] = met;
      ++touched;
      if (stopped) {
        ++s;
        break;
      }
    }
    __threadfence();                                     // meet[] written above is read by the scan of the next round
  }
  if (lane == 0 && touched) atomicAdd(counters, touched);
}

// final flags, in place in lnk[]: link decisions before meet[s], a cut at meet[s], speculation behind it
__global__ __launch_bounds__(256) void k_seg_merge(int64_t n_stripes, const int64_t *st_begin, const int64_t *meet,
                                                   const uint8_t *spec, uint8_t *lnk) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_stripes) return;
  const int64_t a = st_begin[s], b = st_begin[s + 1], m = meet[s];
  for (int64_t i = (m > a ? m : a) + lane; i < b; i += 64) lnk[i] = i == m ? 1 : spec[i];
}

// comp = prev without maxLen: flag[i] = data rule of rows i, i - 1 (table starts are set by k_seg_mark_starts)
__global__ __launch_bounds__(256) void k_seg_prev_flags(SegParams p, int64_t total, uint8_t *flag) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step)
    flag[i] = i > 0 && seg_rule(p.packed, p.KW, p.cutw, p.thresh, i, i - 1) ? 1 : 0;
}

// table holding row i: the last t with off[t] <= i
__device__ inline int64_t seg_table_of(int64_t n_tables, const int64_t *off, int64_t i) {
  int64_t lo = 0, hi = n_tables;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// fixLen: a cut at every multiple of fixLen inside each table (segmentTracks.py:247-248)
__global__ __launch_bounds__(256) void k_seg_fixlen(int64_t total, int64_t n_tables, const int64_t *off,
                                                    int64_t fixLen, uint8_t *flag) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const int64_t rel = i - off[seg_table_of(n_tables, off, i)];
    flag[i] = rel % fixLen == 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_seg_mark_starts(int64_t n_tables, const int64_t *off, uint8_t *flag) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tables) flag[off[t]] = 1;
}

// ---- compaction of the flags into ascending offsets (the three passes of the mask compaction above) -----------------
__global__ __launch_bounds__(256) void k_seg_count(int64_t total, const uint8_t *flag, unsigned *block_cnt) {
  __shared__ unsigned wsum[4];
  const int64_t base = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK;
  unsigned c = 0;
  for (int q = 0; q < 8; ++q) {
    const int64_t i = base + q * 256 + threadIdx.x;
    if (i < total && flag[i]) ++c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// cut_row[rank] = row (over the concatenated tables), cut_rel[rank] = row - start of its table; the rank of every
// table's first row goes to tbl_rank[t] (n_cuts[t] = tbl_rank[t + 1] - tbl_rank[t])
__global__ __launch_bounds__(256) void k_seg_scatter(int64_t total, const uint8_t *flag, const unsigned *block_cnt,
                                                     int64_t n_tables, const int64_t *off, int64_t *cut_row,
                                                     int64_t *cut_rel, int64_t *tbl_rank) {
  __shared__ unsigned wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * TEHMM_SCAN_BLOCK + (int64_t)threadIdx.x * 8;
  unsigned c[8], mine = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c[q] = (i0 + q < total && flag[i0 + q] != 0) ? 1u : 0u;
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
  if (mine == 0) return;
  int64_t t = seg_table_of(n_tables, off, i0);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (!c[q]) continue;
    const int64_t i = i0 + q;
    while (t + 1 < n_tables && off[t + 1] <= i) ++t;
    cut_row[rank] = i;
    cut_rel[rank] = i - off[t];
    if (i == off[t]) tbl_rank[t] = rank;
    ++rank;
  }
}

// ---- the --stats numbers (segmentTracks.py:268-274) ------------------------------------------------------------------
// One thread per cut that is not a table start: the differing tracks D against the true reference row (the previous
// cut in first mode, row i - 1 in prev mode); hist[j][|D|] += 1 for j in D.  Cuts made by maxLen are skipped.
__global__ __launch_bounds__(256) void k_seg_stats(SegParams p, int K, int prev, int64_t n_cuts, const int64_t *cut_row,
                                                   const int64_t *cut_rel, unsigned long long *hist) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_cuts; r += step) {
    if (cut_rel[r] == 0) continue;
    const int64_t i = cut_row[r], last = cut_row[r - 1];
    if (p.maxLen > 0 && i - last >= p.maxLen) continue;
    const uint32_t *a = p.packed + i * p.KW, *b = p.packed + (prev ? i - 1 : last) * p.KW;
    int dif = 0;
    for (int w = 0; w < p.KW; ++w) dif += seg_nz_bytes(a[w] ^ b[w]);
    for (int w = 0; w < p.KW; ++w) {
      const uint32_t x = a[w] ^ b[w];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((x >> (8 * q)) & 0xffu) atomicAdd(&hist[(int64_t)(4 * w + q) * (K + 1) + dif], 1ull);
    }
  }
}

}  // namespace tehmm
