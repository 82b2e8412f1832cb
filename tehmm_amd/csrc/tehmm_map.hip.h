// tehmm_map.hip.h -- maximum-posterior decoding (BaseHMM._decode_map, basehmm.py:332-359) as a row reduction over the
// device-resident posterior rows [rows][N] fp64:
//   path[r]    = np.argmax(post[r])  -- the lowest index among equal maxima (+0.0 == -0.0 is a tie); a row that holds a
//                NaN yields the index of its first NaN (NumPy's rule: a NaN is the maximum);
//   rowmax[r]  = post[r][path[r]]    (NaN for a NaN row);
//   masksum[r] = sum_j post[r][j] * mask[j] in the summation order of k_post_masksum / k_post_masksum_large (bit-equal
//                results), when a mask is given: --maxPost --pd then reads every posterior byte once.
// One wave per row, reads coalesced over the lanes.  The tie rule needs no (value, index) exchange: the wave agrees on the
// maximum VALUE with the fmax butterfly, and the winner is the lowest index among the lanes that hold that value -- a
// ballot and a find-first-set at N <= 128 (the two ballots are in index order: lanes 0..63 hold states 0..63 and then
// 64..127), an integer min over the lanes' own first hits in the strided kernel.  Only the winning lane writes.
//   k_interval_sum: map_logprob[i] = sum of rowmax over interval i ("logprob" of the reference, quirk Q13): one workgroup
//                   per interval, every thread adds its rows in ascending order, then one fixed tree (butterfly in the
//                   wave, the four wave sums in order) -- no atomics, the same bits on every call.
#pragma once
#include "tehmm_kernels.hip.h"

namespace tehmm {

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

// N <= 128: lane = state, at most two values per lane
template <bool MASK>
__global__ __launch_bounds__(256) void k_post_argmax(int64_t rows, int N, const double *post, const double *mask,
                                                     int64_t *path, double *rowmax, double *masksum) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const bool in0 = lane < N, in1 = lane + 64 < N;
  double mk[2] = {0.0, 0.0};
  if (MASK) {
    mk[0] = in0 ? mask[lane] : 0.0;
    mk[1] = in1 ? mask[lane + 64] : 0.0;
  }
  for (int64_t r = wid; r < rows; r += nw) {
    const double v0 = in0 ? post[r * N + lane] : -INFINITY;
    const double v1 = in1 ? post[r * N + lane + 64] : -INFINITY;
    if (MASK) {
      double g = in0 ? v0 * mk[0] : 0.0;
      if (in1) g += v1 * mk[1];
      g = wave_sum_f64(g);
      if (lane == 0) masksum[r] = g;
    }
    unsigned long long b0 = __ballot(v0 != v0), b1 = __ballot(v1 != v1);
    if (!(b0 | b1)) {
      const double m = wave_max_f64(fmax(v0, v1));
      b0 = __ballot(in0 && v0 == m);
      b1 = __ballot(in1 && v1 == m);
    }
    const int idx = b0 ? __ffsll((long long)b0) - 1 : 64 + __ffsll((long long)b1) - 1;
    if (lane == (idx & 63)) {
      path[r] = idx;
      if (rowmax) rowmax[r] = idx < 64 ? v0 : v1;
    }
  }
}

// any N <= 1024: the lanes stride the states
template <bool MASK>
__global__ __launch_bounds__(256) void k_post_argmax_large(int64_t rows, int N, const double *post, const double *mask,
                                                           int64_t *path, double *rowmax, double *masksum) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wid; r < rows; r += nw) {
    double best = -INFINITY, g = 0.0;
    int bidx = INT_MAX;          // this lane's first maximum; once `best` is a NaN no comparison is true: its first NaN
    for (int j = lane; j < N; j += 64) {
      const double v = post[r * N + j];
      if (MASK) g += v * mask[j];
      if (bidx == INT_MAX || v > best || (v != v && best == best)) {
        best = v;
        bidx = j;
      }
    }
    if (MASK) {
      g = wave_sum_f64(g);
      if (lane == 0) masksum[r] = g;
    }
    int idx;
    if (__ballot(best != best)) {
      idx = wave_min_i32(best != best ? bidx : INT_MAX);
    } else {
      const double m = wave_max_f64(best);
      idx = wave_min_i32(best == m ? bidx : INT_MAX);
    }
    if (bidx == idx) {
      path[r] = idx;
      if (rowmax) rowmax[r] = best;
    }
  }
}

// out[i] = sum of vals[off[i] .. off[i + 1]) in one fixed order
__global__ __launch_bounds__(256) void k_interval_sum(const int64_t *off, const double *vals, double *out) {
  __shared__ double part[4];
  const int64_t r0 = off[blockIdx.x], r1 = off[blockIdx.x + 1];
  double s = 0.0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) s += vals[r];
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

}  // namespace tehmm
