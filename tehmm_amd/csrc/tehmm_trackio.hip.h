// tehmm_trackio.hip.h -- painting BED records and FASTA bases into uint8 [T, K] track tables (trackIO.readBedData /
// readFastaData of the reference) as device kernels.
//
// The reference paints record after record, so the last record (in sorted order) that covers a row wins it.  Stated as
// a search: row p of a track takes its value from the largest i with start[i] <= p < end[i]; that is sym0[i] when
// p == start[i] and sym[i] otherwise, and the track's fill value when no record covers p.  start is sorted, so the
// candidates are the prefix [0, j], j = upper_bound(start, p) - 1, and what is wanted is the last entry of that prefix
// whose end lies above p.  Two small structures over end answer that without walking the records, both with fan-out
// 64 and one array per level:
//   * block maxima: level l + 1 holds the maximum of every 64 entries of level l.  To find the last entry above p, scan
//     what is left of j's block backwards, then go up one level and scan the block maxima before it, and so on; at the
//     first maximum above p come back down, in every block to its last entry above p.  At most 64 entries per level
//     both ways, read eight at a time, whatever the overlap depth and however long a record is;
//   * running maxima inside every block of every level: the maximum of end[0 .. j] is then one entry per level, so a
//     row that nothing covers -- most rows of most tracks -- costs that and no search at all.
// Rows whose covering record is the one that starts last cost one load of end.
//
//   k_trk_level       block maxima and in-block running maxima of one level, all tracks in one launch; the first level
//                     also checks the records (sorted starts, 0 <= start < end <= T) and reports the lowest offender
//   k_trk_tile_index  per track and tile, the number of records that start before the tile (a binary search each), so
//                     that the paint never searches more than the records starting inside its tile
//   k_trk_paint       one workgroup per tile of TEHMM_TRACKIO_TILE rows: a lane owns TEHMM_TRACKIO_RUN consecutive rows
//                     of one track (j and the winner are carried from row to row), the [rows][K] tile is put together
//                     in LDS and leaves with 16-byte stores
#pragma once
#include "tehmm_segment.hip.h"

namespace tehmm {

#define TEHMM_TRACKIO_TILE 256       // rows of a tile (LDS: 256 * K bytes, K <= 128)
#define TEHMM_TRACKIO_RUN 8          // consecutive rows of one track a lane paints
#define TEHMM_TRACKIO_FAN 64         // entries under one block maximum
#define TEHMM_TRACKIO_MAX_LEVELS 6   // the sixth level of 2^31 - 1 records is one entry
#define TEHMM_TRACKIO_MAX_TRACKS 128

// index of the track whose range [base[k], base[k + 1]) holds x (empty ranges are skipped)
__device__ inline int trk_owner(const int64_t *base, int K, int64_t x) {
  int lo = 0, hi = K;      // base[lo] <= x < base[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One wave per block of 64 entries of `in`: out[out_base[k] + b] = their maximum, run[in_base[k] + 64 b + t] = the
// maximum of the block's entries 0 .. t.  in / run are indexed alike, as are the bases of out.  CHECK (the first
// level, in = rec_end): every record is looked at once here, so this is where the list is validated; *viol takes the
// lowest offending record index.
template <bool CHECK>
__global__ __launch_bounds__(256) void k_trk_level(int K, int64_t T, const int64_t *in,
                                                   const int64_t *__restrict__ in_base,
                                                   const int64_t *__restrict__ start, int64_t *run, int64_t *out,
                                                   const int64_t *__restrict__ out_base,
                                                   unsigned long long *__restrict__ viol) {
  const int lane = threadIdx.x & 63;
  const int64_t n_out = out_base[K] - out_base[0];
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < n_out; o += waves) {
    const int k = trk_owner(out_base, K, out_base[0] + o);
    const int64_t b = out_base[0] + o - out_base[k];
    const int64_t cnt = in_base[k + 1] - in_base[k];
    const int64_t local = b * TEHMM_TRACKIO_FAN + lane;
    const int64_t i = in_base[k] + local;
    int64_t v = INT64_MIN;
    if (local < cnt) {
      v = in[i];
      if (CHECK) {
        const int64_t s = start[i];
        if (s < 0 || s >= v || v > T || (local > 0 && start[i - 1] > s)) atomicMin(viol, (unsigned long long)i);
      }
    }
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t w = __shfl_up(v, d, 64);
      if (lane >= d && w > v) v = w;
    }
    if (local < cnt) run[i] = v;
    const int64_t top = __shfl(v, 63, 64);
    if (lane == 0) out[out_base[k] + b] = top;
  }
}

struct TrkLevels {
  int n;                                              // levels above the records; the last one is one entry per track
  const int64_t *ptr[TEHMM_TRACKIO_MAX_LEVELS + 1];   // [0] = rec_end, [l] = block maxima of level l - 1
  const int64_t *run[TEHMM_TRACKIO_MAX_LEVELS + 1];   // [l]: in-block running maxima of ptr[l], indexed alike
  const int64_t *base[TEHMM_TRACKIO_MAX_LEVELS + 1];  // [l][K + 1]: first entry of track k in ptr[l]
};

// maximum of end[0 .. j] of track k: one running maximum per level
__device__ inline int64_t trk_prefix_max(const TrkLevels &lv, int k, int64_t j) {
  int64_t acc = INT64_MIN, x = j;
  for (int l = 0; l < lv.n && x >= 0; ++l) {
    const int64_t r = lv.run[l][lv.base[l][k] + x];
    acc = r > acc ? r : acc;
    x = (x >> 6) - 1;                          // the blocks before this one, as entries of the next level
  }
  return acc;
}

// largest t in [lo, x] with v[t] > p, or lo - 1: eight independent loads a round (indices below lo read v[lo] again)
__device__ inline int64_t trk_scan_back(const int64_t *v, int64_t x, int64_t lo, int64_t p) {
  for (int64_t t = x; t >= lo; t -= 8) {
    int64_t a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = v[t - u > lo ? t - u : lo];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (a[u] > p) return t - u > lo ? t - u : lo;
  }
  return lo - 1;
}

// largest i <= hi (an index into track k's records) with end[i] > p, or -1
__device__ inline int64_t trk_last_above(const TrkLevels &lv, int k, int64_t hi, int64_t p) {
  int l = 0;
  int64_t x = hi, t = -1;
  for (;;) {                                  // up: entries <= x of level l, back to the start of x's block
    const int64_t lo = x & ~(int64_t)(TEHMM_TRACKIO_FAN - 1);
    t = trk_scan_back(lv.ptr[l] + lv.base[l][k], x, lo, p);
    if (t >= lo) break;
    x = (x >> 6) - 1;
    if (x < 0 || l + 1 >= lv.n) return -1;
    ++l;
  }
  while (l > 0) {                             // down: the last child above p (its parent's maximum says there is one)
    --l;
    const int64_t cnt = lv.base[l][k + 1] - lv.base[l][k];
    const int64_t lo = t * TEHMM_TRACKIO_FAN;
    const int64_t c = lo + TEHMM_TRACKIO_FAN - 1 < cnt - 1 ? lo + TEHMM_TRACKIO_FAN - 1 : cnt - 1;
    t = trk_scan_back(lv.ptr[l] + lv.base[l][k], c, lo, p);
    if (t < lo) t = lo;                       // (cannot happen on block maxima; keeps the index inside the block)
  }
  return t;
}

// first index in [lo, hi) of a (sorted) with a[index] > p
__device__ inline int64_t trk_upper_bound(const int64_t *a, int64_t lo, int64_t hi, int64_t p) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// index[k * (n_tiles + 1) + t] = records of track k that start before row t * TEHMM_TRACKIO_TILE
__global__ __launch_bounds__(256) void k_trk_tile_index(int K, int64_t n_tiles, const int64_t *__restrict__ rec_base,
                                                        const int64_t *__restrict__ start,
                                                        int32_t *__restrict__ index) {
  const int64_t per = n_tiles + 1, total = per * K;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(x / per);
    const int64_t t = x - k * per;
    const int64_t n = rec_base[k + 1] - rec_base[k];
    index[x] = (int32_t)trk_upper_bound(start + rec_base[k], 0, n, t * TEHMM_TRACKIO_TILE - 1);
  }
}

struct TrkTracks {
  int64_t T;
  int K;
  const uint8_t *fill, *kind;       // [K]
  const int64_t *rec_base;          // [K + 1]
  const int64_t *start, *end;
  const uint8_t *sym0, *sym;
  const int32_t *tile_index;        // [K][n_tiles + 1], k_trk_tile_index
  const uint8_t *seq;               // sequence track q: seq + q * seq_stride (stride a multiple of 8, zero padded)
  int64_t seq_stride;
  const int32_t *seq_rank;          // [K] q of a sequence track
  const uint8_t *lut;               // [n sequence tracks][256]
};

// the winner of row p among records 0 .. j of track k (j >= 0), or -1
__device__ inline int64_t trk_winner(const TrkLevels &lv, int k, const int64_t *en, int64_t j, int64_t p) {
  if (en[j] > p) return j;
  if (j == 0 || !(trk_prefix_max(lv, k, j - 1) > p)) return -1;
  return trk_last_above(lv, k, j - 1, p);
}

__global__ __launch_bounds__(256) void k_trk_paint(TrkTracks tr, TrkLevels lv, int64_t n_tiles,
                                                   uint8_t *__restrict__ data) {
  extern __shared__ __attribute__((aligned(16))) uint8_t trk_tile[];      // [TEHMM_TRACKIO_TILE][K]
  constexpr int RUNS = TEHMM_TRACKIO_TILE / TEHMM_TRACKIO_RUN;
  const int K = tr.K;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * TEHMM_TRACKIO_TILE;
    const int rows = (int)(tr.T - r0 < TEHMM_TRACKIO_TILE ? tr.T - r0 : TEHMM_TRACKIO_TILE);
    for (int it = threadIdx.x; it < K * RUNS; it += blockDim.x) {
      const int k = it / RUNS, q0 = (it % RUNS) * TEHMM_TRACKIO_RUN;
      if (q0 >= rows) continue;
      const int nq = rows - q0 < TEHMM_TRACKIO_RUN ? rows - q0 : TEHMM_TRACKIO_RUN;
      const uint8_t fill = tr.fill[k];
      uint8_t val[TEHMM_TRACKIO_RUN];
      if (tr.kind[k]) {
        const int q = tr.seq_rank[k];
        // r0 + q0 and the stride are multiples of 8 and the buffer is padded: one aligned 8-byte load
        const unsigned long long w =
            *reinterpret_cast<const unsigned long long *>(tr.seq + (int64_t)q * tr.seq_stride + r0 + q0);
        const uint8_t *lut = tr.lut + (int64_t)q * 256;
#pragma unroll
        for (int u = 0; u < TEHMM_TRACKIO_RUN; ++u) {
          const unsigned b = (unsigned)(w >> (8 * u)) & 255u;
          val[u] = b ? lut[b] : fill;
        }
      } else {
        const int64_t *st = tr.start + tr.rec_base[k];
        const int64_t *en = tr.end + tr.rec_base[k];
        // records [lo, hi) start inside this tile: j, the last record starting at or before a row, lies in [lo - 1, hi)
        const int64_t lo = tr.tile_index[(int64_t)k * (n_tiles + 1) + tile];
        const int64_t hi = tr.tile_index[(int64_t)k * (n_tiles + 1) + tile + 1];
        // (trk_walk_run of tehmm_scaling.hip.h is a copy of this walk for the kernels there: change the two together)
        int64_t j = -2, w = -1;      // w: the row's winner or -1
#pragma unroll
        for (int u = 0; u < TEHMM_TRACKIO_RUN; ++u) {
          val[u] = fill;
          if (u >= nq || hi == 0) continue;                     // (hi == 0: no record starts at or before these rows)
          const int64_t p = r0 + q0 + u;
          bool moved = false;
          if (j == -2) {
            j = trk_upper_bound(st, lo, hi, p) - 1;
            moved = true;
          } else if (j + 1 < hi && st[j + 1] <= p) {
            j = trk_upper_bound(st, j + 2, hi, p) - 1;
            moved = true;
          }
          if (moved) w = j < 0 ? -1 : trk_winner(lv, k, en, j, p);
          else if (w >= 0 && !(en[w] > p)) w = w > 0 ? trk_winner(lv, k, en, w - 1, p) : -1;
          if (w >= 0) val[u] = st[w] == p ? tr.sym0[tr.rec_base[k] + w] : tr.sym[tr.rec_base[k] + w];
        }
      }
#pragma unroll
      for (int u = 0; u < TEHMM_TRACKIO_RUN; ++u)
        if (u < nq) trk_tile[(q0 + u) * K + k] = val[u];
    }
    __syncthreads();
    // rows r0 .. r0 + rows of [T, K] are one contiguous piece, 16-byte aligned at its start (r0 * K, r0 % 256 == 0)
    const int bytes = rows * K;
    uint8_t *dst = data + r0 * K;
    const int wide = bytes >> 4;
    for (int c = threadIdx.x; c < wide; c += blockDim.x)
      reinterpret_cast<uint4 *>(dst)[c] = reinterpret_cast<const uint4 *>(trk_tile)[c];
    for (int c = (wide << 4) + threadIdx.x; c < bytes; c += blockDim.x) dst[c] = trk_tile[c];
    __syncthreads();
  }
}

}  // namespace tehmm
