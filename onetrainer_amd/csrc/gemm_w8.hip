// GEMMs over a frozen e4m3 weight (weight_dtype FLOAT_8, LinearFp8.py), gfx950, and the quantiser that makes it.
//
//   forward   Y [M][N] = X [M][K]  dq(W8)^T (+ bias[N]) (+ residual[M][N])
//   dgrad     dX[M][K] = dY[M][N]  dq(W8)   (+ residual[M][K])
//   dq(W8)[n][k] = bf16( bf16(W8[n][k]) * bf16(scale[n]) )     W8 [N][K] OCP e4m3 bytes, K contiguous, scale fp32 [N]
//
// dq is what LinearFp8.forward multiplies by (weight.to(bf16).mul_(scale)): e4m3 -> fp32 is exact, the product of a
// 4-bit and an 8-bit significand is exact in fp32, and one round-to-nearest-even to bf16 is torch's bf16 multiply.
// The scale is applied here, per row, never in the epilogue, so a fused q|k|v weight view stays one GEMM.
//
// Split: one workgroup of 4 waves per 128 x 128 output tile, waves 2 x 2, 64 x 64 each as 4 x 4 blocks of
// v_mfma_f32_16x16x32_bf16 (64 fp32 accumulator registers); the contraction runs in 64-deep steps, in order, in one
// workgroup: no split-K, no atomics, the same bits on every run.
//
// Data movement, per step, two LDS stages of 32 KiB:
//   activations (X / dY, rows of 64 contraction elements)  HBM -> LDS by LDS-DMA (dma16), the K-mode image of
//       gemm.h (128-byte rows, 16-byte chunk c of row r at c ^ (r & 7), swizzle applied on the source address);
//       the descriptor's range check zero-fills rows past M and chunks past the contraction's end;
//   weights  HBM -> registers by two 16-byte loads per lane (16 e4m3 each, predicated on the row and the 16-group
//       being inside the matrix: a byte outside is a finite e4m3 value, so it is never loaded), v_cvt_pk_f32_fp8,
//       v_pk_mul_f32 by the row's scale (as compiled), v_cvt_pk_bf16_f32, two ds_write_b128 into
//         forward: the K-mode image [128 n][64 k]           (read by frag_k2, ds_read_b128)
//         dgrad:   the MN-mode image [64 n][128 k], 32-byte block b of row n at b ^ mn_swz(n)
//                                                            (read by frag_mn2, ds_read_b64_tr_b16)
//       the half of a lane's 32 bytes that goes out first alternates with the row, so the 16 lanes of one write
//       cycle cover all 64 banks.
// Order of one step: DMA and weight loads of tile j+1 are issued, tile j is multiplied (32 MFMAs per wave), then the
// weight registers of tile j+1 are converted and stored, one barrier.  The intent is that this VALU work runs while
// the matrix pipe drains and under the co-resident workgroup's MFMAs; that is supposed, not observed: the kernel was
// not profiled.
//
// What bounds the tile (hipcc -O3, gfx950, --save-temps): LDS 65536 bytes per workgroup = 2 stages x (16 KiB
// activations + 16 KiB weights), so two workgroups share a CU's 160 KiB: 8 waves per CU, 2 per SIMD; a 256-wide tile
// would leave one.  Registers as compiled: forward 123 VGPRs, dgrad 151, no AGPRs, no scratch; at 2 waves per SIMD
// the limit is 256, so registers do not bound it, LDS does.
#include "gemm2_kernel.h"   // frag_k2 / frag_mn2 (the bf16 fragment readers), kimg_off, mn_swz; mfma_prims.h

namespace {

constexpr int BT = 128;            // output tile, both ways
constexpr int BK = 64;             // contraction step
constexpr int NTHREADS = 256;
constexpr int IMG = BT * BK * 2;   // one operand image: 16 KiB
constexpr int STAGE = 2 * IMG;

struct W8Args {
  const bf16_t* a; long long lda;          // X [M][K] (forward) or dY [M][N] (dgrad)
  const uint8_t* w; long long ldw;         // W8 [N][K], row stride in bytes
  const float* scale;                      // [N]
  const bf16_t* bias;                      // [N], forward only
  const bf16_t* residual; long long ldr;   // the output's shape
  bf16_t* out; long long ldo;
  int M, N, K;
};

// 16 e4m3 bytes -> 16 bf16 of (value * s), s already rounded to bf16
__device__ __forceinline__ void dequant16(const uint4& q, float s, uint4& lo, uint4& hi) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const auto f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    o[2 * i] = (uint32_t)f2bf(f0[0] * s) | ((uint32_t)f2bf(f0[1] * s) << 16);
    o[2 * i + 1] = (uint32_t)f2bf(f1[0] * s) | ((uint32_t)f2bf(f1[1] * s) << 16);
  }
  lo = make_uint4(o[0], o[1], o[2], o[3]);
  hi = make_uint4(o[4], o[5], o[6], o[7]);
}

// c ? a : b per register (a select of the whole tuple goes through scratch)
__device__ __forceinline__ uint4 pick4(int c, const uint4& a, const uint4& b) {
  return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// DGRAD = false: contraction over k, output columns n.  DGRAD = true: contraction over n, output columns k.
template <bool DGRAD>
__global__ void __launch_bounds__(NTHREADS, 2) gemm_w8_kernel(W8Args p, unsigned a_bytes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int KC = DGRAD ? p.N : p.K;    // contraction length
  const int NO = DGRAD ? p.K : p.N;    // output columns
  const int tiles_m = (p.M + BT - 1) / BT;
  const int m0 = (blockIdx.x % tiles_m) * BT, c0 = (blockIdx.x / tiles_m) * BT;
  const int nk = (KC + BK - 1) / BK;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1;

  // activations: 16 DMA pieces of 8 rows per image, 4 per wave; lane -> row 8 j + lane / 8, the logical chunk that
  // the swizzle puts at physical chunk lane % 8
  const __amdgpu_buffer_rsrc_t ra = rsrc(p.a, a_bytes);
  const int achunk = (lane & 7) ^ ((lane >> 3) & 7);
  unsigned arow[4];   // element offset of the row, OFF_INVALID past M
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 8 * (wave + 4 * i) + (lane >> 3);
    arow[i] = m < p.M ? (unsigned)(m * (int)p.lda) : OFF_INVALID;
  }
  auto issue_a = [&](char* img, int k0) {
    const int k = k0 + 8 * achunk;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dma16(ra, img + (wave + 4 * i) * 1024, (arow[i] != OFF_INVALID && k < KC) ? (arow[i] + k) * 2u : OFF_INVALID);
  };

  // weights: two 16-byte loads per lane and step.  Forward: load q = tid + 256 i is 16-group q % 4 of tile row q / 4
  // (row n fixed per lane: its scale is read once).  Dgrad: 16-group q % 8 of contraction row q / 8.
  constexpr int GPR = DGRAD ? 8 : 4;   // 16-groups per tile row
  int wrow[2], wgrp[2];
  float wscale[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = threadIdx.x + NTHREADS * i;
    wrow[i] = q / GPR;
    wgrp[i] = q % GPR;
    if constexpr (!DGRAD)
      if (c0 + wrow[i] < p.N) wscale[i] = rbf(p.scale[c0 + wrow[i]]);
  }
  uint4 wq[2];
  auto load_w = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = DGRAD ? k0 + wrow[i] : c0 + wrow[i];
      const int k = DGRAD ? c0 + 16 * wgrp[i] : k0 + 16 * wgrp[i];
      const bool ok = n < p.N && k < p.K;   // K % 16 == 0: a 16-group is inside or outside as a whole
      wq[i] = make_uint4(0u, 0u, 0u, 0u);
      if constexpr (DGRAD) wscale[i] = 0.f;
      if (ok) {
        wq[i] = *reinterpret_cast<const uint4*>(p.w + (long long)n * p.ldw + k);
        if constexpr (DGRAD) wscale[i] = rbf(p.scale[n]);
      }
    }
  };
  auto store_w = [&](char* img) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint4 lo, hi;
      dequant16(wq[i], wscale[i], lo, hi);   // zero bytes stay +0 (0 * finite scale)
      const int r = wrow[i];
      int off, sel;
      if constexpr (DGRAD) {
        off = r * (BT * 2) + ((wgrp[i] ^ mn_swz(r)) << 5);
        sel = r & 1;
      } else {
        off = kimg_off(r, 2 * wgrp[i]);      // chunk 2 g + 1 lands at off ^ 16
        sel = (r >> 1) & 1;
      }
      *reinterpret_cast<uint4*>(img + (off ^ (sel << 4))) = pick4(sel, hi, lo);
      *reinterpret_cast<uint4*>(img + (off ^ (sel << 4) ^ 16)) = pick4(sel, lo, hi);
    }
  };

  float4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};

  issue_a(smem, 0);
  load_w(0);
  store_w(smem + IMG);
  WAIT_VM();
  BARRIER_LDS();

  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * STAGE;
    char* nxt = smem + ((kt + 1) & 1) * STAGE;
    const bool more = kt + 1 < nk;   // workgroup-uniform
    // tile kt + 1: its stage was last read in step kt - 1, before that step's barrier
    if (more) {
      issue_a(nxt, (kt + 1) * BK);
      load_w((kt + 1) * BK);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        fb[j] = DGRAD ? frag_mn2<BT * 2>(cur + IMG, wn * 64 + j * 16, 32 * h) : frag_k2(cur + IMG, wn * 64 + j * 16, 32 * h);
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag_k2(cur, wm * 64 + i * 16, 32 * h);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) store_w(nxt + IMG);
    WAIT_VM();       // the DMA of tile kt + 1 (inline asm: the compiler does not count it)
    BARRIER_LDS();   // publishes tile kt + 1; every read of tile kt has retired
  }

  // lane: row m = block row + lane % 16, four consecutive output columns 4 (lane / 16) ..
  const int g = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + (lane & 15);
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + wn * 64 + j * 16 + 4 * g;
      if (c >= NO) continue;   // NO % 4 == 0: a group of four is inside or outside as a whole
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (!DGRAD && p.bias) {
        const uint2 b = *reinterpret_cast<const uint2*>(p.bias + c);
        v[0] += bf2f((bf16_t)b.x); v[1] += bf2f((bf16_t)(b.x >> 16));
        v[2] += bf2f((bf16_t)b.y); v[3] += bf2f((bf16_t)(b.y >> 16));
      }
      if (p.residual) {
        const uint2 r = *reinterpret_cast<const uint2*>(p.residual + (long long)m * p.ldr + c);
        v[0] += bf2f((bf16_t)r.x); v[1] += bf2f((bf16_t)(r.x >> 16));
        v[2] += bf2f((bf16_t)r.y); v[3] += bf2f((bf16_t)(r.y >> 16));
      }
      uint2 o;
      o.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
      o.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
      *reinterpret_cast<uint2*>(p.out + (long long)m * p.ldo + c) = o;
    }
  }
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <bool DGRAD>
int launch_w8(const W8Args& p, hipStream_t s) {
  const int KC = DGRAD ? p.N : p.K, NO = DGRAD ? p.K : p.N;
  if (!p.a || !p.w || !p.scale || !p.out || p.M < 1 || p.N < 1 || p.K < 1) return OTAMD_EINVAL;
  if (p.K % 16 || p.N % 8 || p.ldw % 16 || p.ldw < p.K) return OTAMD_EINVAL;
  if (p.lda % 8 || p.lda < KC || p.ldo % 4 || p.ldo < NO) return OTAMD_EINVAL;
  if (!aligned16(p.a) || !aligned16(p.w) || !aligned16(p.out) || ((uintptr_t)p.scale & 3)) return OTAMD_EINVAL;
  if (p.bias && ((uintptr_t)p.bias & 7)) return OTAMD_EINVAL;
  if (p.residual && (((uintptr_t)p.residual & 7) || p.ldr % 4 || p.ldr < NO)) return OTAMD_EINVAL;
  const long long a_bytes = ((long long)(p.M - 1) * p.lda + KC) * 2;   // the DMA's 32-bit byte offsets
  if (a_bytes >= (1ll << 31)) return OTAMD_EUNSUPPORTED;
  const long long tiles = (long long)((p.M + BT - 1) / BT) * ((NO + BT - 1) / BT);
  if (tiles >= (1ll << 31)) return OTAMD_EUNSUPPORTED;
  // 64 KiB of dynamic LDS; set on every launch: the attribute belongs to the current device
  if (hipFuncSetAttribute((const void*)gemm_w8_kernel<DGRAD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          2 * STAGE) != hipSuccess)
    return OTAMD_ELAUNCH;
  hipLaunchKernelGGL(gemm_w8_kernel<DGRAD>, dim3((unsigned)tiles), dim3(NTHREADS), 2 * STAGE, s, p, (unsigned)a_bytes);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// ---- quantiser (LinearFp8.quantize) ---------------------------------------------------------------------------------
constexpr int QBLOCKS = 1024;   // the most partial maxima (otamd_quantize_fp8's workspace, floats)

template <bool F32>
__device__ __forceinline__ void load16(const void* w, long long e, float* f) {
  if constexpr (F32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(w) + e)[i];
      f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
    }
  } else {
    const bf8* q = reinterpret_cast<const bf8*>(reinterpret_cast<const bf16_t*>(w) + e);
    unpack8(q[0], f);
    unpack8(q[1], f + 8);
  }
}

// pass 1: part[block] = max |w| over the block's 16-element groups (a maximum does not depend on the order).
// fmaxf drops NaNs: a weight that holds one gets the finite scale of its other elements (torch's abs().max() would
// make the scale NaN); the NaN itself still converts to an e4m3 NaN byte.
template <bool F32>
__global__ void __launch_bounds__(256) absmax_kernel(const void* w, long long groups, float* part) {
  __shared__ float red[4];
  float mx = 0.f;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    float f[16];
    load16<F32>(w, gi * 16, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, fabsf(f[i]));
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// pass 2: scale = max(absmax, 1e-12) / 448; w8 = e4m3_rne(w / scale), saturating at +-448.  A bf16 weight's quotient
// is rounded to bf16 first, as torch's in-place weight.div_(scale) leaves it.
template <bool F32>
__global__ void __launch_bounds__(256) quantize_kernel(const void* w, long long groups, const float* part, int nparts,
                                                       uint8_t* w8, float* scale_rows, long long rows) {
  __shared__ float red[4];
  float mx = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) mx = fmaxf(mx, part[i]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  const float scale = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), 1e-12f) / 448.f;
  if (blockIdx.x == 0)
    for (long long r = threadIdx.x; r < rows; r += 256) scale_rows[r] = scale;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    float f[16];
    load16<F32>(w, gi * 16, f);
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q[j] = f[4 * i + j] / scale;
        if constexpr (!F32) q[j] = rbf(q[j]);
        q[j] = fminf(fmaxf(q[j], -448.f), 448.f);
      }
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], pk, true);
      o[i] = (uint32_t)pk;
    }
    *reinterpret_cast<uint4*>(w8 + gi * 16) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

template <bool F32>
int launch_quantize(const void* w, long long rows, long long cols, uint8_t* w8, float* scale_rows, float* ws,
                    hipStream_t s) {
  const long long groups = rows * cols / 16;
  const int blocks = (int)((groups + 255) / 256 < QBLOCKS ? (groups + 255) / 256 : QBLOCKS);
  hipLaunchKernelGGL(absmax_kernel<F32>, dim3(blocks), dim3(256), 0, s, w, groups, ws);
  OTAMD_CHECK_LAUNCH();
  hipLaunchKernelGGL(quantize_kernel<F32>, dim3(blocks), dim3(256), 0, s, w, groups, (const float*)ws, blocks, w8,
                     scale_rows, rows);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

}  // namespace

OTAMD_API int otamd_linear_w8(const void* x, long long ldx, const void* w8, long long ldw, const float* scale,
                              const void* bias, const void* residual, long long ldr, void* y, long long ldy, int M,
                              int N, int K, hipStream_t s) {
  const W8Args p{(const bf16_t*)x, ldx, (const uint8_t*)w8, ldw, scale, (const bf16_t*)bias, (const bf16_t*)residual,
                 ldr, (bf16_t*)y, ldy, M, N, K};
  return launch_w8<false>(p, s);
}

OTAMD_API int otamd_linear_w8_dgrad(const void* dy, long long lddy, const void* w8, long long ldw, const float* scale,
                                    const void* residual, long long ldr, void* dx, long long lddx, int M, int N, int K,
                                    hipStream_t s) {
  const W8Args p{(const bf16_t*)dy, lddy, (const uint8_t*)w8, ldw, scale, nullptr, (const bf16_t*)residual, ldr,
                 (bf16_t*)dx, lddx, M, N, K};
  return launch_w8<true>(p, s);
}

OTAMD_API int otamd_quantize_fp8(const void* w, int w_f32, long long rows, long long cols, void* w8, float* scale_rows,
                                 float* ws, hipStream_t s) {
  if (!w || !w8 || !scale_rows || !ws || rows < 1 || cols < 16 || cols % 16) return OTAMD_EINVAL;
  if (!aligned16(w) || !aligned16(w8) || ((uintptr_t)scale_rows & 3) || ((uintptr_t)ws & 3)) return OTAMD_EINVAL;
  return w_f32 ? launch_quantize<true>(w, rows, cols, (uint8_t*)w8, scale_rows, ws, s)
               : launch_quantize<false>(w, rows, cols, (uint8_t*)w8, scale_rows, ws, s);
}
