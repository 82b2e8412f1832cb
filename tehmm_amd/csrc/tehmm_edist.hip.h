// tehmm_edist.hip.h -- the emission distribution of a batch (MultitrackHmm.emissionDistribution, hmm.py:265-277) and the
// masked emission column of teHmmEval --ed (teHmmEval.py:273-275), from the packed observation rows a batch already
// holds and the emission rows of a model handle; any N from 1 to 1024:
//   x[r][j]   = ((0 + tab[0][j][obs[r][0]] + ... + tab[K-1][j][obs[r][K-1]]) * normalize) * ratio[r]   (emis_log's order;
//               a symbol past a track's last one reads the zero row), all zero for the rows before the first emittable
//               row OF THEIR INTERVAL (quirk Q9, _emission.pyx:73-80: the reference calls the function once per table);
//   frame     : out[r - row0][j] = x[r][j];
//   column    : out[r - row0]    = log(sum_j exp(x[r][j]) * mask[j]), the reference's plain form without a max shift; a
//               sum that underflows to 0 gives -inf as NumPy does.
// Two kernels, no atomics on results:
//   k_edist_first : first[i] = lowest row of interval i that some state can emit (x > -1e20), len[i] when there is none.
//                   An unsigned integer atomicMin per emittable row seen: a minimum does not depend on the order or on the
//                   launch geometry.  Rows at or behind a minimum that is already known are skipped, so the pass costs
//                   about one row per wave unless an interval cannot be emitted at all.
//   k_edist<W, SPL, COL>: the rows.  A wave owns 64 consecutive rows of the request at a time.  Lane l first finds row l's
//                   interval (a binary search of the 64 lanes side by side), its internal position and its Q9 flag; then
//                   the rows go through W-lane groups, 64 / W rows per step (W = 64 above 32 states; 32, 16 or 8 below,
//                   so that a small model does not leave half or more of the lanes idle).  A group reads its packed row
//                   ONCE, as one coalesced load of K/4 words over its first lanes; the word of four tracks then comes
//                   from a cross-lane read, not from memory again.  Lane = state within the group, SPL states per lane and
//                   pass (strided by W; 1 up to W states, 2 up to 128, 4 above) so that one symbol decode serves SPL
//                   table reads in flight.  Column mode: lane l keeps the sum of row l, and the wave writes its 64
//                   results with one coalesced 512-byte store after taking the 64 logarithms in one go.
#pragma once
#include "tehmm_kernels.hip.h"

namespace tehmm {

template <int W>
__device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// lane l: interval, row within it and internal position of concatenation row r (0 <= r < out0[n])
__device__ __forceinline__ void edist_locate(const IntervalTab &iv, int64_t r, int &id, int64_t &t, int64_t &gpos) {
  int lo = 0, hi = iv.n;                  // first index whose out0 is > r (out0[n] = total > r)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (iv.out0[mid] > r) hi = mid;
    else lo = mid + 1;
  }
  id = lo - 1;
  t = r - iv.out0[id];
  gpos = iv.pos0[id] + t;
}

// SPL states (u + jb, u + jb + W, ...) of the row whose packed words the group's first KPW lanes hold in `wrd`
template <int W, int SPL>
__device__ __forceinline__ void edist_row(const EmisTab &e, uint32_t wrd, double ratio, int u, int jb, int N,
                                          double (&x)[SPL]) {
#pragma unroll
  for (int s = 0; s < SPL; ++s) x[s] = 0.0;
  for (int k0 = 0; k0 < e.K; k0 += 4) {
    const uint32_t w = (uint32_t)__shfl((int)wrd, k0 >> 2, W);
    const int kn = min(4, e.K - k0);
    for (int kk = 0; kk < kn; ++kk) {
      const int k = k0 + kk;
      const int sym = (int)((w >> (kk * 8)) & 0xffu);
      const int trow = sym < e.rowcnt[k] ? e.rowbase[k] + sym : e.zero_row;
      const double *tr = e.tab + (int64_t)trow * e.NP;
#pragma unroll
      for (int s = 0; s < SPL; ++s) {
        const int j = jb + u + W * s;
        if (j < N) x[s] += tr[j];
      }
    }
  }
#pragma unroll
  for (int s = 0; s < SPL; ++s) x[s] *= e.normalize;
  if (e.ratios) {
#pragma unroll
    for (int s = 0; s < SPL; ++s) x[s] *= ratio;
  }
}

// first[i] starts at len[i]; rows [rowA, rowB) of the concatenation (rowA is the start of an interval)
__global__ __launch_bounds__(256) void k_edist_first(IntervalTab iv, EmisTab em, int N, int64_t rowA, int64_t rowB,
                                                     unsigned long long *first) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t rows = rowB - rowA, chunks = (rows + 63) >> 6;
  for (int64_t c = wid; c < chunks; c += nw) {
    const int nr = (int)min((int64_t)64, rows - c * 64);
    int id;
    int64_t t, gpos;
    edist_locate(iv, rowA + c * 64 + min(lane, nr - 1), id, t, gpos);
    const bool known = __hip_atomic_load(&first[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned long long)t;
    if (__ballot(!known) == 0) continue;
    int found = -1;                        // the interval this wave has just settled itself
    for (int q = 0; q < nr; ++q) {
      const int idq = __shfl(id, q);
      if (__shfl((int)known, q) || idq == found) continue;
      const int64_t gq = __shfl((long long)gpos, q), tq = __shfl((long long)t, q);
      const uint32_t wrd = lane < em.KPW ? em.obs32[gq * em.KPW + lane] : 0u;
      const double ratio = em.ratios ? em.ratios[gq] : 1.0;
      bool any = false;
      for (int jb = 0; jb < N; jb += 128) {
        double x[2];
        edist_row<64, 2>(em, wrd, ratio, lane, jb, N, x);
        any = any || (jb + lane < N && x[0] > -1e20) || (jb + lane + 64 < N && x[1] > -1e20);
      }
      if (__ballot(any)) {
        if (lane == 0) atomicMin(&first[idq], (unsigned long long)tq);
        found = idq;
      }
    }
  }
}

// rows [row0, row1) of the concatenation; out: COL ? [row1 - row0] : [row1 - row0][N]
template <int W, int SPL, bool COL>
__global__ __launch_bounds__(256) void k_edist(IntervalTab iv, EmisTab em, int N, int64_t row0, int64_t row1,
                                               const unsigned long long *first, const double *mask, double *out) {
  constexpr int RPS = 64 / W;              // rows per step
  const int lane = threadIdx.x & 63;
  const int u = lane & (W - 1), grp = lane / W;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t rows = row1 - row0, chunks = (rows + 63) >> 6;
  for (int64_t c = wid; c < chunks; c += nw) {
    const int nr = (int)min((int64_t)64, rows - c * 64);
    int id;
    int64_t t, gpos;
    edist_locate(iv, row0 + c * 64 + min(lane, nr - 1), id, t, gpos);
    const int lead = (unsigned long long)t < first[id];      // Q9: a row before its interval's first emittable row
    double res = 0.0;
    for (int q0 = 0; q0 < nr; q0 += RPS) {
      const int q = q0 + grp, qq = min(q, nr - 1);          // (a group past the end repeats the last row and writes nothing)
      const int64_t gq = __shfl((long long)gpos, qq);
      const bool zero = __shfl(lead, qq) != 0;
      const uint32_t wrd = u < em.KPW ? em.obs32[gq * em.KPW + u] : 0u;
      const double ratio = em.ratios ? em.ratios[gq] : 1.0;
      double g = 0.0;
      for (int jb = 0; jb < N; jb += W * SPL) {
        double x[SPL];
        edist_row<W, SPL>(em, wrd, ratio, u, jb, N, x);
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          const int j = jb + u + W * s;
          if (j < N) {
            const double v = zero ? 0.0 : x[s];
            if (COL) g += exp(v) * mask[j];
            else if (q < nr) out[((c * 64 + q) * (int64_t)N) + j] = v;
          }
        }
      }
      if (COL) {
        g = group_sum_f64<W>(g);
        const double mine = RPS == 1 ? g : __shfl(g, (lane % RPS) * W);    // row l went through group l % RPS at step l / RPS
        if (lane / RPS == q0 / RPS) res = mine;
      }
    }
    if (COL && lane < nr) out[c * 64 + lane] = log(res);
  }
}

}  // namespace tehmm
