// tehmm_cyk.hip.h -- CYK decode of the stochastic context free grammar model (cfg.py:219-304, _cfg.pyx:16-89;
// DESIGN.md section 5t).  dp[i][j][x] is the best log probability of state x deriving positions i..j of an interval:
//
//   split   (logProbs1[x][r1][r2] + dp[i][k][r1]) + dp[k+1][j][r2]              k = i .. j-1, every listed (r1, r2)
//   pair    (((logProbs2[x][r] + dp[i+1][j-1][r]) + em[i][x]) + em[j][x]) + logPriors[x][match]      size > 2
//   init    dp[i][i][x] = em[i][x] (single states), dp[i][i+1][x] = (em[i][x] + em[i+1][x]) + logPriors[x][match] (pair states)
//
// The cell is the maximum of its candidates, each rounded in the order written (the library is built with
// -ffp-contract=off); a maximum does not depend on the order of the visits, so the fill keeps no winner.  The traceback
// recomputes, for the at most L - 1 cells of the derivation that are longer than one position, which candidate the
// reference's strict `>` scan (q outer, k inner, pair productions last) would have kept: the first one, in that order,
// that equals the cell.
//
// Layout: one L x L square per (interval, state).  Row i holds dp[i][j] at column j >= i; row j holds the same cell at
// column i < j.  So dp[i][k] (k = i..) and dp[k+1][j] (read from row j, columns k+1..) are both unit-stride in k, and
// the square is no larger than the reference's dp.  Every cell is stored twice (once on the diagonal).
//
//   k_cyk_init     -inf everywhere, the emission rows on the diagonal of single states
//   k_cyk_fill<T>  one launch per diagonal: a group of T lanes per (cell, state), k strided over the lanes.  T <= 64:
//                  256 / T groups per workgroup, reduced by lane exchange; T = 256: the workgroup is one group.
//   k_cyk_score    score and first arg-max of log_start + dp[0][L-1]
//   k_cyk_trace    one workgroup per interval walks the derivation with a stack in global memory
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tehmm {

#define TEHMM_CYK_MAX_STATES 64

struct CykModel {                 // device pointers
  int M;
  int defSym;
  const uint8_t *is_nest;         // [M]
  const int32_t *h1_off;          // [M + 1] into the split list of each left state, ascending (r1, r2)
  const uint8_t *h1_r1, *h1_r2;
  const double *h1_lp;
  const int32_t *h2_off;          // [M + 1] into the pair list, ascending r
  const uint8_t *h2_r;
  const double *h2_lp;
  const double *logPriors;        // [M][2]
  const double *log_start;        // [M]
  const double *em;               // [total][M]
  const uint16_t *al;             // [total] or NULL
};

struct CykItem {                  // one interval; the list is sorted by L, longest first
  int64_t row0;                   // first row of the interval in em / al / trace
  int64_t dp0;                    // first element of its M squares
  int32_t L;
  int32_t idx;                    // position in the caller's order
};

__device__ __forceinline__ double cyk_split(double lp, double a, double b) { return (lp + a) + b; }
__device__ __forceinline__ double cyk_pair(double lp, double inner, double ei, double ej, double prior) {
  return (((lp + inner) + ei) + ej) + prior;
}
__device__ __forceinline__ int cyk_match(const CykModel &m, int64_t row0, int i, int j) {
  if (!m.al) return 0;
  const int a = m.al[row0 + i];
  return a != m.defSym && a == (int)m.al[row0 + j];
}
// the size-2 cell of a pair state before any production is tried
__device__ __forceinline__ double cyk_pair_init(const CykModel &m, int64_t row0, int i, int x) {
  const double *e = m.em + (row0 + i) * m.M + x;
  return (e[0] + e[m.M]) + m.logPriors[2 * x + cyk_match(m, row0, i, i + 1)];
}

__global__ __launch_bounds__(256) void k_cyk_init(CykModel m, const CykItem *items, double *dp) {
  const CykItem it = items[blockIdx.y];
  const int64_t L = it.L, LL = L * L, n = LL * m.M;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int x = (int)(e / LL);
    const int64_t rem = e - x * LL, i = rem / L, j = rem - i * L;
    double v = -INFINITY;
    if (i == j && !m.is_nest[x]) v = m.em[(it.row0 + i) * m.M + x];
    dp[it.dp0 + e] = v;
  }
}

template <int TPC>
__global__ __launch_bounds__(256) void k_cyk_fill(CykModel m, const CykItem *items, int item0, int size, double *dp) {
  const CykItem it = items[item0 + blockIdx.y];
  const int L = it.L, M = m.M;
  constexpr int GPB = 256 / TPC;
  const int64_t g = (int64_t)blockIdx.x * GPB + threadIdx.x / TPC;
  const int lane = threadIdx.x % TPC;
  if (g >= (int64_t)(L - size + 1) * M) return;      // (a whole group leaves together; TPC = 256: the whole workgroup)
  const int i = (int)(g / M), x = (int)(g - (int64_t)i * M), j = i + size - 1;
  const int64_t LL = (int64_t)L * L;
  double *S = dp + it.dp0;
  double best = -INFINITY;
  for (int q = m.h1_off[x]; q < m.h1_off[x + 1]; ++q) {
    const double lp = m.h1_lp[q];
    const double *A = S + m.h1_r1[q] * LL + (int64_t)i * L;      // dp[i][k][r1] at A[k]
    const double *B = S + m.h1_r2[q] * LL + (int64_t)j * L;      // dp[k+1][j][r2] at B[k+1]
    for (int k = i + lane; k < j; k += TPC) best = fmax(best, cyk_split(lp, A[k], B[k + 1]));
  }
  if (size == 2) {
    if (lane == 0 && m.is_nest[x]) best = fmax(best, cyk_pair_init(m, it.row0, i, x));
  } else {
    const double ei = m.em[(it.row0 + i) * M + x], ej = m.em[(it.row0 + j) * M + x];
    const double prior = m.logPriors[2 * x + cyk_match(m, it.row0, i, j)];
    for (int q = m.h2_off[x] + lane; q < m.h2_off[x + 1]; q += TPC)
      best = fmax(best, cyk_pair(m.h2_lp[q], S[m.h2_r[q] * LL + (int64_t)(i + 1) * L + (j - 1)], ei, ej, prior));
  }
#pragma unroll
  for (int off = (TPC < 64 ? TPC : 64) / 2; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
  if (TPC > 64) {
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    best = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
  }
  if (lane == 0) {
    S[x * LL + (int64_t)i * L + j] = best;
    S[x * LL + (int64_t)j * L + i] = best;
  }
}

__global__ void k_cyk_score(CykModel m, const CykItem *items, int n, const double *dp, double *scores, int64_t *top) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const CykItem it = items[t];
  const int64_t L = it.L, LL = L * L;
  double best = 0.0;
  int arg = 0;
  for (int x = 0; x < m.M; ++x) {
    const double v = m.log_start[x] + dp[it.dp0 + x * LL + (L - 1)];
    if (x == 0 || v > best) {
      best = v;
      arg = x;
    }
  }
  scores[it.idx] = best;
  top[it.idx] = arg;
}

// status [4] per interval (caller's order): {code, i, j, state}; code 1: a cell without a winner, 2: internal
// stack: 3 x int32 per entry, L + 1 entries per interval from entry row0 + idx
__global__ __launch_bounds__(256) void k_cyk_trace(CykModel m, const CykItem *items, const double *dp, const int64_t *top,
                                                   int32_t *stack, double *trace, int32_t *status) {
  const CykItem it = items[blockIdx.x];
  const int L = it.L, M = m.M, tid = threadIdx.x;
  const int64_t LL = (int64_t)L * L;
  const double *S = dp + it.dp0;
  int32_t *stk = stack + 3 * (it.row0 + it.idx);
  double *tr = trace + it.row0;
  int32_t *st = status + 4 * (int64_t)it.idx;
  __shared__ int s_sp, s_fail, s_cur[3];
  __shared__ unsigned long long s_key;
  for (int t = tid; t < L; t += 256) tr[t] = -1.0;
  if (tid == 0) {
    s_sp = 0;
    s_fail = 0;
    const int x = (int)top[it.idx];
    if (L == 1) {
      tr[0] = x;
    } else {
      stk[0] = 0;
      stk[1] = L - 1;
      stk[2] = x;
      s_sp = 1;
    }
  }
  for (;;) {
    __syncthreads();
    if (s_sp == 0 || s_fail) break;
    __syncthreads();
    if (tid == 0) {
      const int32_t *e = stk + 3 * (--s_sp);
      s_cur[0] = e[0];
      s_cur[1] = e[1];
      s_cur[2] = e[2];
      s_key = ~0ull;
    }
    __syncthreads();
    const int i = s_cur[0], j = s_cur[1], x = s_cur[2], size = j - i + 1;      // size >= 2
    const double V = S[x * LL + (int64_t)i * L + j];
    // the size-2 cell of a pair state starts as the pair emission: a split replaces it only when strictly above
    bool pair2 = false;
    if (size == 2 && m.is_nest[x]) pair2 = V == -INFINITY || cyk_pair_init(m, it.row0, i, x) == V;
    const bool dead = V == -INFINITY && !pair2;
    if (!pair2 && !dead) {
      bool found = false;
      for (int q = m.h1_off[x]; q < m.h1_off[x + 1] && !found; ++q) {
        const double lp = m.h1_lp[q];
        const double *A = S + m.h1_r1[q] * LL + (int64_t)i * L;
        const double *B = S + m.h1_r2[q] * LL + (int64_t)j * L;
        for (int k = i + tid; k < j; k += 256)
          if (cyk_split(lp, A[k], B[k + 1]) == V) {
            atomicMin(&s_key, ((unsigned long long)(unsigned)(q - m.h1_off[x]) << 32) | (unsigned)k);
            found = true;
            break;
          }
      }
    }
    __syncthreads();
    if (tid == 0) {
      int code = 0;
      int c[2][3];
      int nc = 0;
      if (dead) {
        code = 1;
      } else if (pair2) {
        tr[i] = x;
        tr[j] = x;
      } else if (s_key != ~0ull) {
        const int q = m.h1_off[x] + (int)(s_key >> 32), k = (int)(s_key & 0xffffffffu);
        c[0][0] = i, c[0][1] = k, c[0][2] = m.h1_r1[q];
        c[1][0] = k + 1, c[1][1] = j, c[1][2] = m.h1_r2[q];
        nc = 2;
      } else {
        code = 2;
        if (size > 2) {
          const double ei = m.em[(it.row0 + i) * M + x], ej = m.em[(it.row0 + j) * M + x];
          const double prior = m.logPriors[2 * x + cyk_match(m, it.row0, i, j)];
          for (int q = m.h2_off[x]; q < m.h2_off[x + 1]; ++q)
            if (cyk_pair(m.h2_lp[q], S[m.h2_r[q] * LL + (int64_t)(i + 1) * L + (j - 1)], ei, ej, prior) == V) {
              tr[i] = x;
              tr[j] = x;
              c[0][0] = i + 1, c[0][1] = j - 1, c[0][2] = m.h2_r[q];
              nc = 1;
              code = 0;
              break;
            }
        }
      }
      for (int a = 0; a < nc; ++a) {
        if (c[a][0] == c[a][1]) {
          tr[c[a][0]] = c[a][2];
        } else {
          int32_t *e = stk + 3 * (s_sp++);
          e[0] = c[a][0];
          e[1] = c[a][1];
          e[2] = c[a][2];
        }
      }
      if (code) {
        st[0] = code;
        st[1] = i;
        st[2] = j;
        st[3] = x;
        s_fail = 1;
      }
    }
  }
}

}  // namespace tehmm
