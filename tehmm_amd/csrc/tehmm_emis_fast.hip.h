// tehmm_emis_fast.hip.h -- the fast form of the row part of k_emis_gain_lane (tehmm_lane.hip.h).
//
// emis_rows() (tehmm_coop.hip.h) serves every kernel and every model: per position it fetches the observation words
// with lone 4-byte loads right behind the row stores of the position before (on this target the vector memory counter
// counts stores too: the wait for the word is a wait for the acknowledgement of those stores), reloads a track's row
// count and bases from the argument struct with scalar loads, branches on LDS-or-global per track, and its caller
// multiplies by normalize and masks pads and NaN per element.  The one-wave lane kernel spends most of its positions on
// nothing else, so it gets a form of its own for the models that allow it (host: emis_fast_ok):
//   * no ratios, normalize == 1.0, at most 12 tracks (three observation words), every LDS-staged track before every
//     global-table track in track order, N >= NT - 3, NT <= 36, warm-up a multiple of the block length;
//   * the observation rows of a lane's item travel through LDS in blocks of PB positions: behind the last position of
//     block b the loads of block b + 1 (issued a block earlier) are written to the wave's own LDS area and the 16-byte
//     loads of block b + 2 are issued (ObsWindow, the IndexWindow pattern of tehmm_fused.hip.h); positions read their
//     words back with LDS reads -- the position loop waits for vector memory only at that refill and for the
//     global-table gathers, which are issued a whole LDS phase behind the last stores;
//   * a track's row count and base sit in one lane each of two registers (lane k = track k) and come out with
//     v_readlane: no scalar loads; the LDS tracks and the global tracks are two straight loops;
//   * the sum runs in track order into fixed registers, x[j] = 0.0 first as in emis_rows, through two half-row buffers:
//     the loads of the next half row are in flight while the present one is added.
// The arithmetic is emis_rows' own, operation for operation: rows, NaN marking and gains are bit-identical.
#pragma once
#include "tehmm_coop.hip.h"

namespace tehmm {

#define TEHMM_EFAST_PB 4                                        // positions per observation block (a multiple of 4)
#define TEHMM_EFAST_WORDS (TEHMM_EFAST_PB * 3 + 2)              // staged words per lane (+ 2: three words are always read)
#define TEHMM_EFAST_WAVE_BYTES (TEHMM_EFAST_WORDS * 256)        // ... of one wave, word-major: word i of lane l at i * 256 + l * 4
#define TEHMM_EFAST_NT_MAX 36

typedef unsigned int efast_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) unsigned int efast_lds_u32;

// One lane's window on the observation rows of its item.  Blocks are counted from the wave's first position s0 (a
// multiple of PB away from the item's first); a block that lies outside the lane's own range [lo, hi) -- warm-up of a
// lane that does not run, positions behind the item's end, lanes without an item -- reads the item's first block
// instead (as the slow form clamps gpos), so nothing is read outside the intervals' padded rows.  A block that starts
// inside the range ends inside the interval's padding (intervals are padded to 64 positions).
struct ObsWindow {
  const uint32_t *src;       // observation row of the item's position 0 (16-byte aligned: 4 | position)
  unsigned stage;            // LDS byte address of the lane's column in the wave's area
  int KPW, s0, lo, hi;
  efast_u4 r[TEHMM_EFAST_PB * 3 / 4];   // the block on its way (PB * KPW / 4 16-byte pieces)

  __device__ __forceinline__ void request(int blk) {
    const int sb = s0 + blk * TEHMM_EFAST_PB;
    const efast_u4 *p = (const efast_u4 *)(src + (int64_t)((sb >= lo && sb < hi) ? sb : 0) * KPW);
#pragma unroll
    for (int c = 0; c < TEHMM_EFAST_PB * 3 / 4; ++c)
      if (c < TEHMM_EFAST_PB / 4 * KPW) r[c] = p[c];
  }
  __device__ __forceinline__ void commit() {
    efast_lds_u32 *d = (efast_lds_u32 *)(size_t)stage;
#pragma unroll
    for (int c = 0; c < TEHMM_EFAST_PB * 3 / 4; ++c)
      if (c < TEHMM_EFAST_PB / 4 * KPW) {
        d[(4 * c + 0) * 64] = r[c].x;
        d[(4 * c + 1) * 64] = r[c].y;
        d[(4 * c + 2) * 64] = r[c].z;
        d[(4 * c + 3) * 64] = r[c].w;
      }
  }
  // the three words that start at position rel (0 .. PB - 1) of the committed block; words past KPW are never used
  __device__ __forceinline__ void words(int rel, unsigned &w0, unsigned &w1, unsigned &w2) const {
    const efast_lds_u32 *d = (const efast_lds_u32 *)(size_t)(stage + (unsigned)(rel * KPW) * 256u);
    w0 = d[0];
    w1 = d[64];
    w2 = d[128];
  }
};

template <int NT>
struct EmisFastRows {
  static constexpr int H = NT / 4;           // 16-byte pieces of half a row
  static constexpr unsigned ROWB = NT * 8;
  const char *tab;                           // global table
  int meta_cnt;                              // lane k: rowcnt[k]
  unsigned meta_base;                        // lane k: LDS byte address (LDS track) / byte offset into tab of the track's first row
  unsigned zero_lds, zero_glb;               // the zero rows
  int K, n_lds;
  unsigned w0, w1, w2;                       // observation bytes not yet consumed

  __device__ __forceinline__ void init(const EmisTab &em, const double *ltab, int lane) {
    const unsigned la = (unsigned)(size_t)(__attribute__((address_space(3))) const double *)ltab;
    const bool tr = lane < em.K;
    const int lb = tr ? em.ldsbase[lane] : -1;
    meta_cnt = tr ? em.rowcnt[lane] : 0;
    meta_base = lb >= 0 ? la + (unsigned)lb * ROWB : (unsigned)(tr ? em.rowbase[lane] : 0) * ROWB;
    n_lds = __popcll(__ballot(lb >= 0));
    K = em.K;
    tab = (const char *)em.tab;
    zero_lds = la + (unsigned)em.lds_zero * ROWB;
    zero_glb = (unsigned)em.zero_row * ROWB;
  }
  // row address of track k (uniform) for the next observation byte
  __device__ __forceinline__ unsigned row_of(int k, unsigned zero) {
    const unsigned sym = w0 & 0xffu;
    w0 = __builtin_amdgcn_alignbit(w1, w0, 8);
    w1 = __builtin_amdgcn_alignbit(w2, w1, 8);
    w2 >>= 8;
    const unsigned cnt = (unsigned)__builtin_amdgcn_readlane(meta_cnt, k);
    const unsigned base = (unsigned)__builtin_amdgcn_readlane((int)meta_base, k);
    return sym < cnt ? base + sym * ROWB : zero;
  }
  template <int HALF>
  static __device__ __forceinline__ void load_lds(unsigned a, d2v (&buf)[H]) {
    lds_cd2 *p = (lds_cd2 *)(size_t)a;
#pragma unroll
    for (int i = 0; i < H; ++i) buf[i] = p[HALF * H + i];
  }
  template <int HALF>
  __device__ __forceinline__ void load_glb(unsigned off, d2v (&buf)[H]) const {
    const d2v *p = (const d2v *)(tab + off);
#pragma unroll
    for (int i = 0; i < H; ++i) buf[i] = p[HALF * H + i];
  }
  template <int HALF>
  static __device__ __forceinline__ void add(double (&x)[NT], const d2v (&buf)[H]) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
      x[2 * (HALF * H + i)] += buf[i].x;
      x[2 * (HALF * H + i) + 1] += buf[i].y;
    }
  }
  // x = sum of the tracks' rows in track order, from 0.0; w0..w2 hold the position's observation words
  __device__ __forceinline__ void rows(double (&x)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) x[j] = 0.0;
    d2v a[H], b[H];
    if (n_lds > 0) {
      unsigned ra = row_of(0, zero_lds);
      asm volatile("v_mov_b32 %0, %1" : "=v"(ra) : "v"(ra));        // (one register, immediate offsets: see lds_row)
      load_lds<0>(ra, a);
#pragma unroll 1
      for (int k = 1; k < n_lds; ++k) {
        load_lds<1>(ra, b);
        ra = row_of(k, zero_lds);
        asm volatile("v_mov_b32 %0, %1" : "=v"(ra) : "v"(ra));
        add<0>(x, a);
        load_lds<0>(ra, a);
        add<1>(x, b);
      }
      load_lds<1>(ra, b);
      add<0>(x, a);
    }
    if (n_lds < K) {
      // the first global half row goes out before the last LDS half is added
      unsigned ro = row_of(n_lds, zero_glb);
      load_glb<0>(ro, a);
      if (n_lds > 0) add<1>(x, b);
#pragma unroll 1
      for (int k = n_lds + 1; k < K; ++k) {
        load_glb<1>(ro, b);
        ro = row_of(k, zero_glb);
        add<0>(x, a);
        load_glb<0>(ro, a);
        add<1>(x, b);
      }
      load_glb<1>(ro, b);
      add<0>(x, a);
      add<1>(x, b);
    } else {
      add<1>(x, b);
    }
  }
};

}  // namespace tehmm
