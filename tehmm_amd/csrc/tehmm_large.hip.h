// tehmm_large.hip.h -- sequential Viterbi, forward and backward / posterior kernels for 129 <= N <= 1024 states.
//
// One workgroup of 1024 threads (16 waves) per interval, taken in the batch's launch order (iv.order).  The sizes
// decide the layout: at N = 256 the fp64 transition table is 512 KB (LDS is 160 KiB per CU), at N = 1024 it is 8 MB
// (more than one XCD's L2).  So no copy of the table is kept on the CU: every step streams it once from L2 /
// Infinity Cache, each element read by exactly one thread, coalesced along the to-states.
//
// Thread layout (LargeGeom, computed on the host from N):
//   * to-lane tl = tid % TOL, from-group g = tid / TOL (G groups, G * TOL <= 1024, TOL a multiple of 64);
//   * the thread owns the to-states j = tl + TOL * s, s < NS (NS = ceil(N / 256) <= 4), and scans the from-states
//     [g FQ, g FQ + FQ) of the state vector V (LDS, broadcast reads) against the table rows lt[f][j] (global);
//   * partial results of the G groups go through LDS; group 0 combines them in ascending group order and writes the
//     new V.  Two workgroup barriers per step.
// Viterbi candidates are formed exactly as in k_viterbi (-ffp-contract=off, the from = 0 case with ratios, Q4); the
// key is (value, lowest from-index): inside a group the ascending strict '>' scan, across groups ascending order with
// strict '>', which equals the reference's single ascending scan (a NaN start value stays, later NaNs never win).
// Forward / backward are the scaled linear domain of k_forward_wide / k_backward_wide (power-of-two scaling by the
// previous row's largest exponent, log-likelihood from the summed exponents); the group partial sums are added in
// group order (tolerance 1e-6 like every scaled-linear kernel here).
// Emission rows of a block of PBL positions are computed by the 16 waves side by side (one row per wave, lane =
// states lane + 64 q) into an LDS ring before the block's steps; before the first emittable row of an interval the
// block takes a second pass so that the leading-rows quirk (Q9, _emission.pyx:73-80) is applied in order.
//
// LDS (doubles): ring [PBL][NP] | V [NP] | pval [G][NS * TOL] | parg (int) [G][NS * TOL] | ms [16] | red [2][16] |
//                redi (int) [2][16] | flag (int) [16]
#pragma once
#include "tehmm_kernels.hip.h"

#define TEHMM_LARGE_MAX 1024      // largest N of any entry point
#define TEHMM_LARGE_BLOCK 1024    // threads per workgroup
#define TEHMM_LARGE_MS 16         // emission states per lane (NP / 64)

namespace tehmm {

struct LargeGeom {
  int N, NP;        // NP = N rounded up to 64 (row stride of every table)
  int NS, TOL, G, FQ;
  int PBL;          // positions per emission block
};

__host__ __device__ inline LargeGeom large_geom(int N) {
  LargeGeom g;
  g.N = N;
  g.NP = (N + 63) & ~63;
  g.NS = (N + 255) / 256;
  const int per = (N + g.NS - 1) / g.NS;
  g.TOL = (per + 63) & ~63;
  g.G = TEHMM_LARGE_BLOCK / g.TOL;
  g.FQ = (N + g.G - 1) / g.G;
  const int pbl = 8192 / g.NP;
  g.PBL = pbl < 1 ? 1 : (pbl > 16 ? 16 : pbl);
  return g;
}

__host__ __device__ inline size_t large_lds_bytes(const LargeGeom &g) {
  const size_t part = (size_t)g.G * g.NS * g.TOL;
  return ((size_t)g.PBL * g.NP + g.NP + part + 16 + 32) * sizeof(double) + (part + 32 + 16) * sizeof(int);
}

struct LargeLds {
  double *ring, *V, *pval, *ms, *red;
  int *parg, *redi, *flag;
};
__device__ __forceinline__ LargeLds large_lds(double *sm, const LargeGeom &g) {
  LargeLds l;
  const size_t part = (size_t)g.G * g.NS * g.TOL;
  l.ring = sm;
  l.V = l.ring + (size_t)g.PBL * g.NP;
  l.pval = l.V + g.NP;
  l.ms = l.pval + part;
  l.red = l.ms + 16;
  l.parg = (int *)(l.red + 32);
  l.redi = l.parg + part;
  l.flag = l.redi + 32;
  return l;
}

// Emission log row of one position for the states lane + 64 q (q < NP / 64): _emission.pyx:65-72 order (x = 0;
// x += table[k][j][obs[k]] for k ascending; x *= normalize; x *= ratio).  The padding states read zeros.
__device__ __forceinline__ void large_emis_row(const EmisTab &e, int64_t gpos, int lane, int NPW,
                                               double (&x)[TEHMM_LARGE_MS]) {
  const uint32_t *row = e.obs32 + gpos * e.KPW;
#pragma unroll
  for (int q = 0; q < TEHMM_LARGE_MS; ++q) x[q] = 0.0;
  for (int k = 0; k < e.K; ++k) {
    const uint32_t w = row[k >> 2];
    const int sym = (int)((w >> ((k & 3) * 8)) & 0xffu);
    const int trow = sym < e.rowcnt[k] ? e.rowbase[k] + sym : e.zero_row;
    const double *tr = e.tab + (int64_t)trow * e.NP + lane;
#pragma unroll
    for (int q = 0; q < TEHMM_LARGE_MS; ++q)
      if (q < NPW) x[q] += tr[64 * q];
  }
#pragma unroll
  for (int q = 0; q < TEHMM_LARGE_MS; ++q) x[q] *= e.normalize;
  if (e.ratios) {
    const double r = e.ratios[gpos];
#pragma unroll
    for (int q = 0; q < TEHMM_LARGE_MS; ++q) x[q] *= r;
  }
}

__device__ __forceinline__ double large_row_max(const double (&x)[TEHMM_LARGE_MS], int lane, int N, int NPW) {
  double m = -INFINITY;
#pragma unroll
  for (int q = 0; q < TEHMM_LARGE_MS; ++q)
    if (q < NPW && lane + 64 * q < N) m = fmax(m, x[q]);
  return wave_max_f64(m);
}

// MODE 0: the log row into the ring; MODE 1: exp(row - max) into the ring and the max into ms[p]
template <int MODE>
__device__ __forceinline__ void large_emis_store(double (&x)[TEHMM_LARGE_MS], int lane, int N, int NPW, double *dst,
                                                 double *ms, int p) {
  if (MODE == 1) {
    const double m = large_row_max(x, lane, N, NPW);
#pragma unroll
    for (int q = 0; q < TEHMM_LARGE_MS; ++q)
      if (q < NPW) dst[lane + 64 * q] = lane + 64 * q < N ? exp(x[q] - m) : 0.0;
    if (lane == 0 && ms) ms[p] = m;
  } else {
#pragma unroll
    for (int q = 0; q < TEHMM_LARGE_MS; ++q)
      if (q < NPW) dst[lane + 64 * q] = x[q];
  }
}

// Emission rows of the block [t0, t0 + np) of an interval into the ring (one row per wave).  While no emittable row
// has been seen (block-uniform), the raw rows go to the ring first, the first row with max > -1e20 is found through
// the flags, and the rows before it are zeroed in a second pass.  The caller puts a barrier behind.
template <int MODE>
__device__ void large_emis_block(const EmisTab &em, const LargeGeom &lg, const LargeLds &l, int64_t gpos0, int64_t t0,
                                 int np, bool &seen, int64_t &fg) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int N = lg.N, NP = lg.NP, NPW = NP >> 6;
  if (seen) {
    for (int p = w; p < np; p += nw) {
      double x[TEHMM_LARGE_MS];
      large_emis_row(em, gpos0 + p, lane, NPW, x);
      large_emis_store<MODE>(x, lane, N, NPW, l.ring + (size_t)p * NP, l.ms, p);
    }
    return;
  }
  for (int p = w; p < np; p += nw) {
    double x[TEHMM_LARGE_MS];
    large_emis_row(em, gpos0 + p, lane, NPW, x);
    const double m0 = large_row_max(x, lane, N, NPW);
    if (lane == 0) l.flag[p] = m0 > -1e20 ? 1 : 0;
    large_emis_store<0>(x, lane, N, NPW, l.ring + (size_t)p * NP, nullptr, p);
  }
  __syncthreads();
  int first = np;
  for (int p = 0; p < np; ++p)
    if (l.flag[p]) { first = p; break; }
  for (int p = w; p < np; p += nw) {
    double x[TEHMM_LARGE_MS];
    double *row = l.ring + (size_t)p * NP;
#pragma unroll
    for (int q = 0; q < TEHMM_LARGE_MS; ++q)
      if (q < NPW) x[q] = p < first ? 0.0 : row[lane + 64 * q];
    large_emis_store<MODE>(x, lane, N, NPW, row, l.ms, p);
  }
  if (first < np) {
    seen = true;
    fg = t0 + first;
  }
}

// ------------------------------------------------------------------------------------------
// Viterbi.  FRAME: emission rows from frame [T][N] (array-level tehmm_viterbi), else fused from the model's rows
// (decode: no ratios on the emission, Q11).  Pointers: tb[(pos0 + t) * NP + state], PtrT = uint8_t while N <= 256.
// ------------------------------------------------------------------------------------------
template <bool RATIO, bool FRAME, typename PtrT>
__global__ __launch_bounds__(TEHMM_LARGE_BLOCK) void k_vit_large(IntervalTab iv, EmisTab em, LargeGeom lg,
                                                                const double *g_lt, const double *g_pi,
                                                                const double *tratios, const double *frame, PtrT *tb,
                                                                int *last_state, double *logprob) {
  extern __shared__ double sm[];
  const LargeLds l = large_lds(sm, lg);
  const int N = lg.N, NP = lg.NP, NS = lg.NS, TOL = lg.TOL, G = lg.G;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  const int id = iv.order[blockIdx.x];
  const int64_t T = iv.len[id];
  const int64_t p0 = iv.pos0[id];
  if (T <= 0) return;
  const int tl = tid % TOL, g = tid / TOL;
  const int f0 = g * lg.FQ, f1 = min(N, f0 + lg.FQ);
  const int PS = NS * TOL;
  double ltd[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = tl + TOL * s;
    ltd[s] = (s < NS && j < N) ? g_lt[(size_t)j * NP + j] : 0.0;
  }
  const double lt00 = g_lt[0];
  bool seen = false;
  int64_t fg = T;
  for (int64_t t0 = 0; t0 < T; t0 += lg.PBL) {
    const int np = (int)min((int64_t)lg.PBL, T - t0);
    if (FRAME) {
      for (int p = w; p < np; p += nw)
        for (int j = lane; j < NP; j += 64) l.ring[(size_t)p * NP + j] = j < N ? frame[(t0 + p) * N + j] : -INFINITY;
    } else {
      large_emis_block<0>(em, lg, l, p0 + t0, t0, np, seen, fg);
    }
    __syncthreads();
    for (int p = 0; p < np; ++p) {
      const int64_t t = t0 + p;
      const double *b = l.ring + (size_t)p * NP;
      double r = 0.0;
      if (RATIO) r = tratios[p0 + t];
      if (t == 0) {
        if (g == 0) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int j = tl + TOL * s;
            if (s < NS && j < N) {
              double v = g_pi[j] + b[j];
              if (RATIO && r > 1.) v += ltd[s] * (r - 1.);
              l.V[j] = v;
            }
          }
        }
        __syncthreads();
        continue;
      }
      if (g < G) {
        const bool rg = RATIO && r > 1.;
        const double rm1 = r - 1.;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (s >= NS) break;
          const int j = tl + TOL * s;
          const int jj = j < N ? j : 0;
          const double bj = b[jj];
          const double *col = g_lt + jj;
          double best = -INFINITY;
          int arg = f0;
          int f = f0;
          if (g == 0) {
            best = (l.V[0] + col[0]) + bj;
            if (RATIO) {
              best += ltd[s] * r;
              if (j == 0) best -= lt00;
            }
            arg = 0;
            f = 1;
          }
          if (rg) {
            const double addr = ltd[s] * rm1;
#pragma unroll 8
            for (; f < f1; ++f) {
              double c = (l.V[f] + col[(size_t)f * NP]) + bj;
              c += addr;
              if (c > best) { best = c; arg = f; }
            }
          } else {
#pragma unroll 8
            for (; f < f1; ++f) {
              const double c = (l.V[f] + col[(size_t)f * NP]) + bj;
              if (c > best) { best = c; arg = f; }
            }
          }
          l.pval[g * PS + s * TOL + tl] = best;
          l.parg[g * PS + s * TOL + tl] = arg;
        }
      }
      __syncthreads();
      if (g == 0) {
        for (int s = 0; s < NS; ++s) {
          const int j = tl + TOL * s;
          if (j >= N) continue;
          double fin = l.pval[s * TOL + tl];
          int fa = l.parg[s * TOL + tl];
          for (int gg = 1; gg < G; ++gg) {
            const double c = l.pval[gg * PS + s * TOL + tl];
            if (c > fin) { fin = c; fa = l.parg[gg * PS + s * TOL + tl]; }
          }
          l.V[j] = fin;
          tb[(p0 + t) * NP + j] = (PtrT)fa;
        }
      }
      __syncthreads();
    }
  }
  // np.argmax over V[T-1] (first maximum; a NaN wins as soon as it is met)
  if (tid == 0) {
    int last = 0;
    double m = l.V[0];
    if (m == m) {
      for (int j = 1; j < N; ++j) {
        const double x = l.V[j];
        if (x != x) { last = j; break; }
        if (x > m) { m = x; last = j; }
      }
    }
    last_state[id] = last;
    logprob[id] = l.V[last];
  }
}

// Partial sum of one from-group for the to-state j: sum over f in [f0, f1) of V[f] * M[f][j] (M = A forward, AT
// backward), two interleaved accumulators.
__device__ __forceinline__ double large_partial(const double *V, const double *col, int NP, int f0, int f1) {
  double acc0 = 0.0, acc1 = 0.0;
  int f = f0;
#pragma unroll 4
  for (; f + 1 < f1; f += 2) {
    acc0 = fma(V[f], col[(size_t)f * NP], acc0);
    acc1 = fma(V[f + 1], col[(size_t)(f + 1) * NP], acc1);
  }
  if (f < f1) acc0 = fma(V[f], col[(size_t)f * NP], acc0);
  return acc0 + acc1;
}

// ------------------------------------------------------------------------------------------
// Forward pass, scaled linear domain (k_forward_wide): the scaled alpha rows go to post (out0 * N layout), the
// backward kernel turns them into posteriors in place.  No ratios (Q12).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TEHMM_LARGE_BLOCK) void k_fwd_large(IntervalTab iv, EmisTab em, LargeGeom lg,
                                                                const double *g_A, const double *g_pi, double *post,
                                                                double *fwd_logprob, int64_t *first_good) {
  extern __shared__ double sm[];
  const LargeLds l = large_lds(sm, lg);
  const int N = lg.N, NP = lg.NP, NS = lg.NS, TOL = lg.TOL, G = lg.G;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int id = iv.order[blockIdx.x];
  const int64_t T = iv.len[id];
  const int64_t p0 = iv.pos0[id];
  if (T <= 0) return;
  double *out = post + iv.out0[id] * N;
  const int tl = tid % TOL, g = tid / TOL;
  const int f0 = g * lg.FQ, f1 = min(N, f0 + lg.FQ);
  const int PS = NS * TOL, NW0 = TOL / 64;      // the waves of group 0
  bool seen = false;
  int64_t fg = T;
  double Ecum = 0.0, Mcum = 0.0;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t t0 = 0; t0 < T; t0 += lg.PBL) {
    const int np = (int)min((int64_t)lg.PBL, T - t0);
    large_emis_block<1>(em, lg, l, p0 + t0, t0, np, seen, fg);
    __syncthreads();
    for (int p = 0; p < np; ++p) {
      const int64_t t = t0 + p;
      const double *bh = l.ring + (size_t)p * NP;
      Mcum += l.ms[p];
      if (t > 0 && g < G) {
        for (int s = 0; s < NS; ++s) {
          const int j = tl + TOL * s;
          l.pval[g * PS + s * TOL + tl] = large_partial(l.V, g_A + (j < N ? j : 0), NP, f0, f1);
        }
      }
      if (t > 0) __syncthreads();
      if (g == 0) {
        int eprev = 0;
        if (t > 0) {
          const int *re = l.redi + ((t - 1) & 1) * 16;
          eprev = re[0];
          for (int q = 1; q < NW0; ++q) eprev = max(eprev, re[q]);
          Ecum += (double)eprev;
        }
        int e = -1022;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int j = tl + TOL * s;
          if (!(s < NS && j < N)) continue;
          if (t == 0) {
            a[s] = exp(g_pi[j]) * bh[j];
          } else {
            double sum = l.pval[s * TOL + tl];
            for (int gg = 1; gg < G; ++gg) sum += l.pval[gg * PS + s * TOL + tl];
            a[s] = ldexp(sum * bh[j], -eprev);
          }
          l.V[j] = a[s];
          out[t * N + j] = a[s];
          e = max(e, exp_of(a[s]));
        }
        e = wave_max_i32(e);
        if (lane == 0) l.redi[(t & 1) * 16 + w] = e;
      }
      __syncthreads();
    }
  }
  if (g == 0) {
    double tot = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) tot += a[s];      // (slots past NS and states past N hold 0)
    tot = wave_sum_f64(tot);
    if (lane == 0) l.red[w] = tot;
  }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int q = 0; q < NW0; ++q) tot += l.red[q];
    fwd_logprob[id] = log(tot) + Ecum * 0.6931471805599453 + Mcum;
    first_good[id] = fg;
  }
}

// ------------------------------------------------------------------------------------------
// Backward pass + posterior in place (k_backward_wide): beta_t[i] = sum_j A[i][j] w_{t+1}[j] with
// w_{t+1} = bh'_{t+1} * beta_{t+1} (AT rows stream like A), post_t = normalise(alpha_t * beta_t) with the float32 eps
// of score_samples (basehmm.py:265-272).  The normalisation of row t needs a block-wide sum: it is written one phase
// later, behind the barrier that ends the step.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TEHMM_LARGE_BLOCK) void k_bwd_large(IntervalTab iv, EmisTab em, LargeGeom lg,
                                                                const double *g_AT, double *post,
                                                                const int64_t *first_good) {
  extern __shared__ double sm[];
  const LargeLds l = large_lds(sm, lg);
  const int N = lg.N, NP = lg.NP, NS = lg.NS, TOL = lg.TOL, G = lg.G;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  const int id = iv.order[blockIdx.x];
  const int64_t T = iv.len[id];
  const int64_t p0 = iv.pos0[id];
  if (T <= 0) return;
  double *out = post + iv.out0[id] * N;
  const int64_t fg = first_good[id];
  const int tl = tid % TOL, g = tid / TOL;
  const int f0 = g * lg.FQ, f1 = min(N, f0 + lg.FQ);
  const int PS = NS * TOL, NW0 = TOL / 64, NPW = NP >> 6;
  const double eps = 1.1920928955078125e-07;
  const double epsden = 1.0 + (double)N * eps;
  // group 0 carries: beta of the last row, the products g of the row whose posterior is pending (its wave sums and
  // beta exponents are in slot `par` of red / redi), the scaling exponent of the next step
  double beta[4] = {0.0, 0.0, 0.0, 0.0}, gv[4] = {0.0, 0.0, 0.0, 0.0};
  int eprev = 1;                                   // exponent of 1.0 in the frexp convention
  int par = 0;
  int64_t pending = T - 1;
  // position T-1: beta = 1
  if (g == 0) {
    double tot = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = tl + TOL * s;
      if (s < NS && j < N) {
        beta[s] = 1.0;
        gv[s] = out[(T - 1) * N + j];
        tot += gv[s];
      }
    }
    tot = wave_sum_f64(tot);
    if (lane == 0) l.red[w] = tot;
  }
  __syncthreads();
  // posterior of the pending row (its sums are behind the last barrier); the exponent of its beta scales the next step
  auto finish_pending = [&]() {
    double tot = 0.0;
    for (int q = 0; q < NW0; ++q) tot += l.red[par * 16 + q];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = tl + TOL * s;
      if (s < NS && j < N) {
        double pr = gv[s] / tot;
        pr = (pr + eps) / epsden;
        out[pending * N + j] = pr;
      }
    }
    if (pending < T - 1) {
      int e = l.redi[par * 16];
      for (int q = 1; q < NW0; ++q) e = max(e, l.redi[par * 16 + q]);
      eprev = e;
    }
  };
  for (int64_t thi = T - 2; thi >= 0; thi -= lg.PBL) {
    const int np = (int)min((int64_t)lg.PBL, thi + 1);
    for (int p = w; p < np; p += nw) {             // ring[p] <- bh'[(thi - p) + 1]
      const int64_t u = thi - p + 1;
      double x[TEHMM_LARGE_MS];
      large_emis_row(em, p0 + u, lane, NPW, x);
      if (u < fg) {
#pragma unroll
        for (int q = 0; q < TEHMM_LARGE_MS; ++q) x[q] = 0.0;
      }
      large_emis_store<1>(x, lane, N, NPW, l.ring + (size_t)p * NP, nullptr, p);
    }
    __syncthreads();
    if (g == 0) {                                  // w = bh' * beta of the block's first step
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int j = tl + TOL * s;
        if (s < NS && j < N) l.V[j] = l.ring[j] * beta[s];
      }
    }
    __syncthreads();
    for (int p = 0; p < np; ++p) {
      const int64_t t = thi - p;
      if (g < G) {
        for (int s = 0; s < NS; ++s) {
          const int j = tl + TOL * s;
          l.pval[g * PS + s * TOL + tl] = large_partial(l.V, g_AT + (j < N ? j : 0), NP, f0, f1);
        }
      }
      __syncthreads();
      if (g == 0) {
        finish_pending();
        par ^= 1;
        int e = -1022;
        double tot = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int i = tl + TOL * s;
          if (s < NS && i < N) {
            const double av = out[t * N + i];      // scaled alpha row
            double sum = l.pval[s * TOL + tl];
            for (int gg = 1; gg < G; ++gg) sum += l.pval[gg * PS + s * TOL + tl];
            beta[s] = ldexp(sum, -eprev);
            e = max(e, exp_of(beta[s]));
            gv[s] = av * beta[s];
            tot += gv[s];
            if (p + 1 < np) l.V[i] = l.ring[(size_t)(p + 1) * NP + i] * beta[s];
          }
        }
        e = wave_max_i32(e);
        tot = wave_sum_f64(tot);
        if (lane == 0) {
          l.redi[par * 16 + w] = e;
          l.red[par * 16 + w] = tot;
        }
        pending = t;
      }
      __syncthreads();
    }
  }
  if (g == 0) finish_pending();
}

// out[r] = sum_j post[r][j] * mask[j] for any N <= 1024: one wave per row, lanes stride the states
__global__ __launch_bounds__(256) void k_post_masksum_large(int64_t rows, int N, const double *post,
                                                            const double *mask, double *out) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wid; r < rows; r += nw) {
    double g = 0.0;
    for (int j = lane; j < N; j += 64) g += post[r * N + j] * mask[j];
    g = wave_sum_f64(g);
    if (lane == 0) out[r] = g;
  }
}

}  // namespace tehmm
