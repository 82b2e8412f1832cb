// Whole-chip issue rates of the instructions the throughput kernels are made of (diagnostic, not product): what
// `roofline` figures in DESIGN.md are priced against when the bound is arithmetic.
//   hipcc --offload-arch=gfx950 -O3 tools/peak_rates.hip -o tools/peak_rates.bin && tools/peak_rates.bin
// Every kernel: `waves` waves per SIMD on all 1024 SIMDs, each issuing ITER x 16 independent instructions of one
// kind; rate = instructions x flops / HIP-event time.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

#define ITER 4096

// MODE 0: v_mfma_f64_16x16x4_f64 (2048 flop)   1: v_fma_f64 (128 flop per wave instruction)
// MODE 2: v_mfma_f32_32x32x2_f32 (4096 flop)   3: v_mfma_f32_16x16x4_f32 (2048 flop)   4: v_add_f64 + v_max_f64 pairs
// MODE 5: v_fmac_f64_dpp row_newbcast (128 flop)   6: v_permlane32_swap_b32   7: v_permlane16_swap_b32
// MODE 8 / 9: one step of a fused posterior pass at 36 padded states, per iteration (ITER / 4 iterations)
//   8: 9 k-blocks of 2 MFMAs + 4 DPP FMAs, then the reduce-scatter of the four tail sums (6 swaps, 3 adds)
//   9: 9 k-blocks of 3 MFMAs (the padded row tile)
#define DPP_FMA(acc, coef, x, j) \
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #j " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(coef), "v"(x))
__device__ __forceinline__ double rate_lohi(unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); }
template <int MODE>
__global__ __launch_bounds__(256) void k_rate(double *out, double seed) {
  const double a = seed + threadIdx.x * 1e-9, b = 1.0 - 1e-9 * threadIdx.x;
  if (MODE == 0) {
    d4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (d4){0, 0, 0, 0};
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[0] = s;
  } else if (MODE == 1) {
    double x[16];
    for (int i = 0; i < 16; ++i) x[i] = a + i;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = __builtin_fma(x[i], b, a);
    }
    double s = 0;
    for (int i = 0; i < 16; ++i) s += x[i];
    if (s == 12345.678) out[0] = s;
  } else if (MODE == 2) {
    f16v acc[4];
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
    const float fa = (float)a, fb = (float)b;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[i], 0, 0, 0);
    }
    float s = 0;
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 16; ++k) s += acc[i][k];
    if (s == 12345.678f) out[0] = s;
  } else if (MODE == 3) {
    f4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (f4){0, 0, 0, 0};
    const float fa = (float)a, fb = (float)b;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, fb, acc[i], 0, 0, 0);
    }
    float s = 0;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678f) out[0] = s;
  } else if (MODE == 5) {
    double x[16];
    for (int i = 0; i < 16; ++i) x[i] = a + i;
    asm volatile("s_nop 4" ::: "memory");          // (the DPP source is read well behind the VALU that wrote it)
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int i = 0; i < 16; i += 4) {
        DPP_FMA(x[i], a, b, 0);
        DPP_FMA(x[i + 1], a, b, 1);
        DPP_FMA(x[i + 2], a, b, 2);
        DPP_FMA(x[i + 3], a, b, 3);
      }
    }
    double s = 0;
    for (int i = 0; i < 16; ++i) s += x[i];
    if (s == 12345.678) out[0] = s;
  } else if (MODE == 6 || MODE == 7) {
    unsigned x[32];
    for (int i = 0; i < 32; ++i) x[i] = threadIdx.x * 33u + i;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const auto r = MODE == 6 ? __builtin_amdgcn_permlane32_swap(x[2 * i], x[2 * i + 1], false, false)
                                 : __builtin_amdgcn_permlane16_swap(x[2 * i], x[2 * i + 1], false, false);
        x[2 * i] = r[0];
        x[2 * i + 1] = r[1];
      }
    }
    unsigned s = 0;
    for (int i = 0; i < 32; ++i) s += x[i];
    if (s == 12345678u) out[0] = s;
  } else if (MODE == 8 || MODE == 9) {
    constexpr int RM = MODE == 8 ? 2 : 3;
    d4 acc[RM];
    for (int i = 0; i < RM; ++i) acc[i] = (d4){0, 0, 0, 0};
    double tf[RM][9], tl[9], v[9];
    for (int k = 0; k < 9; ++k) {
      for (int i = 0; i < RM; ++i) tf[i][k] = a * (1 + i + 3 * k);
      tl[k] = (threadIdx.x & 15) < 4 ? b * (k + 1) * 1e-3 : 0.0;
      v[k] = b + k;
    }
    double p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    asm volatile("s_nop 4" ::: "memory");
    for (int it = 0; it < ITER / 4; ++it) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int i = 0; i < RM; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(tf[i][k], v[k], acc[i], 0, 0, 0);
        if (MODE == 8) {
          DPP_FMA(p0, tl[k], v[k], 0);
          DPP_FMA(p1, tl[k], v[k], 1);
          DPP_FMA(p2, tl[k], v[k], 2);
          DPP_FMA(p3, tl[k], v[k], 3);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (MODE == 8) {
        const auto al = __builtin_amdgcn_permlane32_swap(__double2loint(p0), __double2loint(p2), false, false);
        const auto ah = __builtin_amdgcn_permlane32_swap(__double2hiint(p0), __double2hiint(p2), false, false);
        const auto bl = __builtin_amdgcn_permlane32_swap(__double2loint(p1), __double2loint(p3), false, false);
        const auto bh = __builtin_amdgcn_permlane32_swap(__double2hiint(p1), __double2hiint(p3), false, false);
        const double r0 = rate_lohi(al[0], ah[0]) + rate_lohi(al[1], ah[1]);
        const double r1 = rate_lohi(bl[0], bh[0]) + rate_lohi(bl[1], bh[1]);
        const auto cl = __builtin_amdgcn_permlane16_swap(__double2loint(r0), __double2loint(r1), false, false);
        const auto ch = __builtin_amdgcn_permlane16_swap(__double2hiint(r0), __double2hiint(r1), false, false);
        p0 = rate_lohi(cl[0], ch[0]) + rate_lohi(cl[1], ch[1]);        // (carried: the next step starts from the tail)
        p1 = p2 = p3 = 0;
      }
    }
    double s = p0 + p1 + p2 + p3;
    for (int i = 0; i < RM; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[0] = s;
  } else {
    double x[8];
    for (int i = 0; i < 8; ++i) x[i] = a + i;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        double t = x[i] + b;
        asm volatile("v_max_f64 %0, %1, %2" : "=v"(x[i]) : "v"(t), "v"(a));
      }
    }
    double s = 0;
    for (int i = 0; i < 8; ++i) s += x[i];
    if (s == 12345.678) out[0] = s;
  }
}

template <int MODE>
static void run(const char *name, double flop_per_instr, int waves_per_simd, double *d_out, bool per_step = false) {
  const int blocks = 256 * waves_per_simd;      // 256 CUs, one 4-wave block per CU and wave slot
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL(k_rate<MODE>, dim3(blocks), dim3(256), 0, 0, d_out, 1.0);
  hipDeviceSynchronize();
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k_rate<MODE>, dim3(blocks), dim3(256), 0, 0, d_out, 1.0);
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  const double waves = (double)blocks * 4.0;
  if (per_step) {                               // MODE 8 / 9: time of one step of one wave, and of a SIMD's waves in turn
    const double steps = (double)(ITER / 4);
    printf("%-28s %d wave(s)/SIMD: %8.3f ms  %7.1f ns per step and wave  %7.1f ns per step and SIMD\n", name, waves_per_simd,
           ms, ms * 1e6 / steps, ms * 1e6 / (steps * waves_per_simd));
    return;
  }
  const double instr_per_wave = (double)ITER * 16.0;
  const double ns_per_instr_per_simd = ms * 1e6 / (instr_per_wave * waves_per_simd);
  printf("%-28s %d wave(s)/SIMD: %8.3f ms  %7.2f TFLOP/s  %6.1f ns per instruction and SIMD\n", name, waves_per_simd, ms,
         instr_per_wave * waves * flop_per_instr / (ms * 1e-3) / 1e12, ns_per_instr_per_simd);
}

int main() {
  double *d_out;
  hipMalloc(&d_out, 64);
  for (int w : {1, 2, 4}) {
    run<0>("v_mfma_f64_16x16x4_f64", 2048.0, w, d_out);
    run<1>("v_fma_f64", 128.0, w, d_out);
    run<4>("v_add_f64 + v_max_f64", 64.0, w, d_out);
    run<2>("v_mfma_f32_32x32x2_f32", 4096.0, w, d_out);
    run<3>("v_mfma_f32_16x16x4_f32", 2048.0, w, d_out);
    run<5>("v_fmac_f64_dpp row_newbcast", 128.0, w, d_out);
    run<6>("v_permlane32_swap_b32", 0.0, w, d_out);
    run<7>("v_permlane16_swap_b32", 0.0, w, d_out);
    run<9>("step: 27 MFMA", 0.0, w, d_out, true);
    run<8>("step: 18 MFMA + 36 DPP + 9", 0.0, w, d_out, true);
  }
  hipFree(d_out);
  return 0;
}
