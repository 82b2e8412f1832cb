// tehmm_scaling.hip.h -- what setTrackScaling needs of a numeric track, on the walk of tehmm_trackio.hip.h (DESIGN.md
// section 5p).  The tool never takes the delta branch, so a row's value is the value of the record that wins it, and
// every statistic of the per-base float array (minimum, maximum, length, histogram counts) is a statistic of the record
// list weighted by the rows each record wins.
//
//   k_trk_rows_won    tile and run geometry of k_trk_paint; a lane turns the winners of its 8 rows into runs of equal
//                     winners, the 32 lanes of a track join runs that continue from lane to lane (one scan over the half
//                     wave), and only the lane in which a run ends adds its length: a record that wins a whole tile costs
//                     at most one 64-bit atomic add for that tile, and none while it goes on winning the workgroup's
//                     tiles.  Rows nobody wins are summed per workgroup in LDS and leave with one add per track and
//                     workgroup.  Integer adds: the result does not depend on their order
//   k_trk_paint_f32   the same walk; writes rec_val[winner] or the track's fill into out[k][T] (track after track)
#pragma once
#include "tehmm_trackio.hip.h"

namespace tehmm {

#define TEHMM_TRACKIO_RUNS (TEHMM_TRACKIO_TILE / TEHMM_TRACKIO_RUN)      // lanes of one track in a tile
#define TEHMM_TRACKIO_PASS (256 / TEHMM_TRACKIO_RUNS)                    // tracks a workgroup walks at a time
static_assert(TEHMM_TRACKIO_RUNS == 32 && TEHMM_TRACKIO_RUN == 8, "the joins below are written for 32 lanes of 8 rows");

// each(u, w) for the rows p0 + u, u < nq, of track k in order, w the winner of the row (index in the track, or -1); p0
// is the first row of a run of tile `tile`.  The walk of k_trk_paint: j and the winner are carried from row to row.
template <typename Each>
__device__ inline void trk_walk_run(const TrkTracks &tr, const TrkLevels &lv, int k, int64_t tile, int64_t n_tiles,
                                    int64_t p0, int nq, Each &&each) {
  const int64_t *st = tr.start + tr.rec_base[k];
  const int64_t *en = tr.end + tr.rec_base[k];
  const int64_t lo = tr.tile_index[(int64_t)k * (n_tiles + 1) + tile];
  const int64_t hi = tr.tile_index[(int64_t)k * (n_tiles + 1) + tile + 1];
  int64_t j = -2, cur = -1;
#pragma unroll
  for (int u = 0; u < TEHMM_TRACKIO_RUN; ++u) {
    if (u >= nq) continue;
    if (hi > 0) {                                         // (hi == 0: no record starts at or before these rows)
      const int64_t p = p0 + u;
      bool moved = false;
      if (j == -2) {
        j = trk_upper_bound(st, lo, hi, p) - 1;
        moved = true;
      } else if (j + 1 < hi && st[j + 1] <= p) {
        j = trk_upper_bound(st, j + 2, hi, p) - 1;
        moved = true;
      }
      if (moved) cur = j < 0 ? -1 : trk_winner(lv, k, en, j, p);
      else if (cur >= 0 && !(en[cur] > p)) cur = cur > 0 ? trk_winner(lv, k, en, cur - 1, p) : -1;
    }
    each(u, (int32_t)cur);                                // (a call holds fewer than 2^31 records)
  }
}

// n rows go to record w of the track whose counters start at `won` (global), or, without a winner, to the workgroup's
// uncovered rows of the track (LDS)
__device__ inline void trk_count(unsigned long long *won, unsigned long long *unc, int32_t w, unsigned long long n) {
  if (w >= 0) atomicAdd(won + w, n);
  else atomicAdd(unc, n);
}

__global__ __launch_bounds__(256) void k_trk_rows_won(TrkTracks tr, TrkLevels lv, int64_t n_tiles,
                                                      unsigned long long *__restrict__ won,
                                                      unsigned long long *__restrict__ uncovered) {
  __shared__ unsigned long long unc[TEHMM_TRACKIO_MAX_TRACKS];
  // the winner of all rows of a track in a tile, and its rows so far: a record over a whole chromosome wins most tiles
  // of every workgroup, and is added once per workgroup, not once per tile.  Entry k belongs to one lane (run 0 of k)
  __shared__ unsigned long long whole_n[TEHMM_TRACKIO_MAX_TRACKS];
  __shared__ int32_t whole_w[TEHMM_TRACKIO_MAX_TRACKS];
  const int K = tr.K;
  const int run = threadIdx.x & (TEHMM_TRACKIO_RUNS - 1), q0 = run * TEHMM_TRACKIO_RUN;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    unc[k] = whole_n[k] = 0;
    whole_w[k] = -1;
  }
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * TEHMM_TRACKIO_TILE;
    const int rows = (int)(tr.T - r0 < TEHMM_TRACKIO_TILE ? tr.T - r0 : TEHMM_TRACKIO_TILE);
    // every lane of a wave takes every turn of this loop (the joins shuffle); lanes without rows carry nq = 0
    for (int k0 = 0; k0 < K; k0 += TEHMM_TRACKIO_PASS) {
      const int k = k0 + (threadIdx.x / TEHMM_TRACKIO_RUNS);
      const int nq = k >= K || q0 >= rows ? 0 : rows - q0 < TEHMM_TRACKIO_RUN ? rows - q0 : TEHMM_TRACKIO_RUN;
      unsigned long long *won_k = won + (k < K ? tr.rec_base[k] : 0), *unc_k = unc + (k < K ? k : 0);
      // the lane's rows as runs of equal winners: the first (hw, hl) and the last (tw, tl) may go on in the lanes
      // beside it, the ones between are added here; uni: the lane's rows are one run.  -2 is no winner's name
      int32_t hw = -2, tw = -2;
      int hl = 0, tl = 0;
      bool uni = true;
      if (nq > 0) {
        trk_walk_run(tr, lv, k, tile, n_tiles, r0 + q0, nq, [&](int u, int32_t w) {
          if (u == 0 || w == tw) {
            tw = w;
            ++tl;
            return;
          }
          if (uni) {
            hw = tw;
            hl = tl;
            uni = false;
          } else {
            trk_count(won_k, unc_k, tw, tl);
          }
          tw = w;
          tl = 1;
        });
        if (uni) {
          hw = tw;
          hl = tl;
        }
      }
      // mostly one winner (or none) has all rows of the track in the tile: no joining, and no add while it stays
      const bool flat = nq == 0 || (uni && hw == __shfl(hw, 0, TEHMM_TRACKIO_RUNS));
      if (__ballot(flat) == ~0ull) {
        if (run == 0 && nq > 0) {
          if (whole_w[k] != hw) {
            trk_count(won_k, unc_k, whole_w[k], whole_n[k]);
            whole_w[k] = hw;
            whole_n[k] = 0;
          }
          whole_n[k] += rows;
        }
        continue;
      }
      // inclusive scan over the track's 32 lanes: (p_hw, p_tw, p_uni, p_tl) describes lanes i - d + 1 .. i joined, p_tl
      // the length of the run that ends with lane i's last row
      int32_t p_hw = hw, p_tw = tw;
      int p_tl = tl, p_uni = uni ? 1 : 0;
      for (int d = 1; d < TEHMM_TRACKIO_RUNS; d <<= 1) {
        const int32_t a_hw = __shfl_up(p_hw, d, TEHMM_TRACKIO_RUNS), a_tw = __shfl_up(p_tw, d, TEHMM_TRACKIO_RUNS);
        const int a_tl = __shfl_up(p_tl, d, TEHMM_TRACKIO_RUNS), a_uni = __shfl_up(p_uni, d, TEHMM_TRACKIO_RUNS);
        if (run >= d) {
          if (p_uni) {
            if (a_tw == p_hw) {
              p_tl += a_tl;
              p_uni = a_uni;
            } else {
              p_uni = 0;
            }
          }
          p_hw = a_hw;
        }
      }
      const int32_t before_tw = __shfl_up(p_tw, 1, TEHMM_TRACKIO_RUNS), next_hw = __shfl_down(hw, 1, TEHMM_TRACKIO_RUNS);
      const int before_tl = __shfl_up(p_tl, 1, TEHMM_TRACKIO_RUNS);
      if (nq > 0) {
        // a first run that ends inside the lane takes what led up to it; the last run is added where it ends
        if (!uni) trk_count(won_k, unc_k, hw, hl + (run > 0 && before_tw == hw ? before_tl : 0));
        if (run == TEHMM_TRACKIO_RUNS - 1 || next_hw != tw) trk_count(won_k, unc_k, tw, p_tl);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    trk_count(won + tr.rec_base[k], unc + k, whole_w[k], whole_n[k]);
    if (unc[k]) atomicAdd(uncovered + k, unc[k]);
  }
}

__global__ __launch_bounds__(256) void k_trk_paint_f32(TrkTracks tr, TrkLevels lv, int64_t n_tiles,
                                                       const float *__restrict__ fill,
                                                       const float *__restrict__ rec_val, float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tilebuf[TEHMM_TRACKIO_PASS][TEHMM_TRACKIO_TILE];
  const int K = tr.K;
  const int g = threadIdx.x / TEHMM_TRACKIO_RUNS, q0 = (threadIdx.x & (TEHMM_TRACKIO_RUNS - 1)) * TEHMM_TRACKIO_RUN;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * TEHMM_TRACKIO_TILE;
    const int rows = (int)(tr.T - r0 < TEHMM_TRACKIO_TILE ? tr.T - r0 : TEHMM_TRACKIO_TILE);
    for (int k0 = 0; k0 < K; k0 += TEHMM_TRACKIO_PASS) {
      const int k = k0 + g;
      if (k < K && q0 < rows) {
        const int nq = rows - q0 < TEHMM_TRACKIO_RUN ? rows - q0 : TEHMM_TRACKIO_RUN;
        const float *val = rec_val + tr.rec_base[k];
        const float f = fill[k];
        float v[TEHMM_TRACKIO_RUN];
#pragma unroll
        for (int u = 0; u < TEHMM_TRACKIO_RUN; ++u) v[u] = f;
        trk_walk_run(tr, lv, k, tile, n_tiles, r0 + q0, nq, [&](int u, int32_t w) { v[u] = w >= 0 ? val[w] : f; });
        float4 *dst = reinterpret_cast<float4 *>(&tilebuf[g][q0]);
        dst[0] = make_float4(v[0], v[1], v[2], v[3]);
        dst[1] = make_float4(v[4], v[5], v[6], v[7]);
      }
      __syncthreads();
      // rows r0 .. r0 + rows of a track are one contiguous piece of out; 16-byte aligned when T is a multiple of 4
      const int nk = K - k0 < TEHMM_TRACKIO_PASS ? K - k0 : TEHMM_TRACKIO_PASS;
      if ((tr.T & 3) == 0) {
        const int wide = rows >> 2;
        for (int c = threadIdx.x; c < nk * wide; c += blockDim.x) {
          const int kk = c / wide, x = c - kk * wide;
          reinterpret_cast<float4 *>(out + (int64_t)(k0 + kk) * tr.T + r0)[x] =
              reinterpret_cast<const float4 *>(tilebuf[kk])[x];
        }
      } else {
        for (int c = threadIdx.x; c < nk * rows; c += blockDim.x) {
          const int kk = c / rows, x = c - kk * rows;
          out[(int64_t)(k0 + kk) * tr.T + r0 + x] = tilebuf[kk][x];
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace tehmm
