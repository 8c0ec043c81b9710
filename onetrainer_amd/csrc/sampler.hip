// Sampling kernels (compiled with -ffp-contract=off: one rounding per written operation, which is what the
// bounds of tests/_oracle_sampler.py count):
//   classifier-free guidance + CFG rescale + one DDIM step (eta = 0)
//                                   modules/modelSampler/StableDiffusionXLSampler.py:156-172 with the DDIMScheduler
//                                   of modules/util/create.py:1255-1266 (clip_sample False)
//   decoder output -> 8-bit RGB     the inverse of image_to_nhwc (VaeImageProcessor.postprocess: denormalize, * 255,
//                                   round)
//
// Layouts: pred / next input are NHWC bf16 with 8 held channels (4 real, one 16-byte chunk per pixel), the latent
// state is NHWC fp32 with 4 channels (one 16-byte chunk per pixel).  One thread owns one pixel: three 16-byte loads,
// three 16-byte stores.
//
// CFG rescale needs the unbiased standard deviation of the guided prediction and of the positive prediction over
// each sample's 4 * h * w real elements.  Pass 1 (cfg_stats_kernel) writes per-workgroup partial sums and sums of
// squares in double (p is formed in double there too, so the statistics carry no fp32 rounding of their own: a
// product of two floats is exact in double); pass 2 sums a sample's partials in a fixed order in every workgroup.
// No atomics, so two runs give the same bits.
#include "common.h"

#define STEP_THREADS 256

struct __align__(16) f32x4 { float v[4]; };

// the 4 real channels of pixel `pix` of a [.., 8] bf16 tensor
__device__ __forceinline__ void load_pred4(const bf16_t* p, long long pix, float* f) {
  const bf8 v = *reinterpret_cast<const bf8*>(p + pix * 8);
  f[0] = __uint_as_float(v.w[0] << 16);
  f[1] = __uint_as_float(v.w[0] & 0xffff0000u);
  f[2] = __uint_as_float(v.w[1] << 16);
  f[3] = __uint_as_float(v.w[1] & 0xffff0000u);
}

// block-wide sum of one double in a fixed order; `red` holds STEP_THREADS / 64 doubles
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < STEP_THREADS / 64; ++i) t += red[i];
  return t;
}

// pass 1: partial[(b * nblk + blk) * 4 + {0, 1, 2, 3}] = sum p, sum p^2, sum pos, sum pos^2 over the block's pixels
__global__ void __launch_bounds__(STEP_THREADS) cfg_stats_kernel(const bf16_t* __restrict__ pred, int B, long long HW,
                                                                 float cfg_scale, double* __restrict__ partial,
                                                                 int nblk) {
  const int b = blockIdx.y;
  const long long pix = (long long)blockIdx.x * STEP_THREADS + threadIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (pix < HW) {
    float ng[4], ps[4];
    load_pred4(pred, (long long)b * HW + pix, ng);
    load_pred4(pred, (long long)(B + b) * HW + pix, ps);
    const double c = (double)cfg_scale;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double n = (double)ng[k], q = (double)ps[k];
      const double p = n + c * (q - n);
      s[0] += p;
      s[1] += p * p;
      s[2] += q;
      s[3] += q * q;
    }
  }
  __shared__ double red[STEP_THREADS / 64];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = block_sum_d(s[k], red);
  if (threadIdx.x == 0) {
    double* o = partial + ((long long)b * nblk + blockIdx.x) * 4;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
  }
}

// pass 2: the guided prediction, its rescale, the DDIM step, the next UNet input.
// partial == nullptr: no rescale (factor 1).  x_out may alias x (each thread reads its pixel before it writes it).
__global__ void __launch_bounds__(STEP_THREADS) cfg_ddim_update_kernel(
    const bf16_t* __restrict__ pred, const float* x, float* x_out, bf16_t* __restrict__ next_in, int B, long long HW,
    float cfg_scale, float cfg_rescale, int v_pred, const float* __restrict__ sqrt_acp,
    const float* __restrict__ sqrt_1m, int t, int t_prev, const double* __restrict__ partial, int nblk) {
  const int b = blockIdx.y;
  __shared__ double red[STEP_THREADS / 64];
  __shared__ float factor_s;
  if (partial) {
    // every workgroup of a sample sums the same partials in the same order: lane-strided, then the fixed tree
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nblk; k += STEP_THREADS) {
      const double* o = partial + ((long long)b * nblk + k) * 4;
      s[0] += o[0]; s[1] += o[1]; s[2] += o[2]; s[3] += o[3];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = block_sum_d(s[k], red);
    if (threadIdx.x == 0) {
      const double n = 4.0 * (double)HW;
      const double var_p = (s[1] - s[0] * s[0] / n) / (n - 1.0);
      const double var_q = (s[3] - s[2] * s[2] / n) / (n - 1.0);
      // a constant guided prediction (var_p == 0, e.g. all zeros) has no deviation to rescale to: the factor is 1
      // there, where the reference's division would turn the whole latent into NaN
      const double ratio = var_p > 0.0 ? sqrt(fmax(var_q, 0.0)) / sqrt(var_p) : 1.0;
      // rescale * ratio + (1 - rescale), written so that ratio == 1 gives exactly 1
      factor_s = (float)(1.0 + (double)cfg_rescale * (ratio - 1.0));
    }
    __syncthreads();
  }
  const long long pix = (long long)blockIdx.x * STEP_THREADS + threadIdx.x;
  if (pix >= HW) return;
  const float factor = partial ? factor_s : 1.f;
  const float sa_t = sqrt_acp[t], s1_t = sqrt_1m[t], sa_p = sqrt_acp[t_prev], s1_p = sqrt_1m[t_prev];
  float ng[4], ps[4];
  load_pred4(pred, (long long)b * HW + pix, ng);
  load_pred4(pred, (long long)(B + b) * HW + pix, ps);
  const long long xi = (long long)b * HW + pix;
  const f32x4 xv = *reinterpret_cast<const f32x4*>(x + xi * 4);
  f32x4 o;
  float nb[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float p = ng[k] + cfg_scale * (ps[k] - ng[k]);
    if (partial) p = p * factor;
    const float xk = xv.v[k];
    float x0, e;
    if (v_pred) {
      x0 = sa_t * xk - s1_t * p;
      e = sa_t * p + s1_t * xk;
    } else {
      x0 = (xk - s1_t * p) / sa_t;
      e = p;
    }
    o.v[k] = sa_p * x0 + s1_p * e;
    nb[k] = o.v[k];
    nb[4 + k] = 0.f;
  }
  *reinterpret_cast<f32x4*>(x_out + xi * 4) = o;
  const bf8 nv = pack8(nb);
  *reinterpret_cast<bf8*>(next_in + xi * 8) = nv;
  *reinterpret_cast<bf8*>(next_in + ((long long)(B + b) * HW + pix) * 8) = nv;
}

// x: bf16 [npix, cpad] (the first 3 channels are R, G, B in [-1, 1]) -> out: uint8 [npix, 3] =
// round(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even, evaluated in double (every step but the last is then exact
// for a bf16 input of ordinary size).  A NaN becomes 0.  One thread writes 4 pixels: 12 bytes as three dwords.
__device__ __forceinline__ uint32_t rgb8_of(bf16_t v) {
  const double y = fmin(fmax((double)bf2f(v) * 0.5 + 0.5, 0.0), 1.0);   // fmax(NaN, 0) = 0
  return (uint32_t)(int)rint(y * 255.0);
}
__global__ void __launch_bounds__(256) nhwc_to_rgb8_kernel(const bf16_t* __restrict__ x, int cpad, long long npix,
                                                           uint8_t* __restrict__ out) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long p0 = g * 4;
  if (p0 >= npix) return;
  uint32_t by[12];
  const int cnt = (int)(npix - p0 < 4 ? npix - p0 : 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < cnt) {
      const bf16_t* px = x + (p0 + i) * cpad;
      if (cpad == 8) {
        const bf8 v = *reinterpret_cast<const bf8*>(px);
        by[3 * i] = rgb8_of((bf16_t)(v.w[0] & 0xffffu));
        by[3 * i + 1] = rgb8_of((bf16_t)(v.w[0] >> 16));
        by[3 * i + 2] = rgb8_of((bf16_t)(v.w[1] & 0xffffu));
      } else {
        by[3 * i] = rgb8_of(px[0]);
        by[3 * i + 1] = rgb8_of(px[1]);
        by[3 * i + 2] = rgb8_of(px[2]);
      }
    } else {
      by[3 * i] = by[3 * i + 1] = by[3 * i + 2] = 0;
    }
  }
  uint8_t* o = out + p0 * 3;
  if (cnt == 4) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);   // p0 * 3 = g * 12: dword aligned when `out` is
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o4[j] = by[4 * j] | (by[4 * j + 1] << 8) | (by[4 * j + 2] << 16) | (by[4 * j + 3] << 24);
  } else {
    for (int j = 0; j < 3 * cnt; ++j) o[j] = (uint8_t)by[j];
  }
}

OTAMD_API long long otamd_cfg_ddim_step_ws_bytes(int B, long long HW) {
  if (B <= 0 || HW <= 0) return 0;
  const long long nblk = (HW + STEP_THREADS - 1) / STEP_THREADS;
  return (long long)B * nblk * 4 * (long long)sizeof(double);
}

OTAMD_API int otamd_cfg_ddim_step(const void* pred, const float* x, float* x_out, void* next_in, int B, long long HW,
                                  float cfg_scale, float cfg_rescale, int v_pred, const float* sqrt_acp,
                                  const float* sqrt_1m, int n_table, int t, int t_prev, void* ws, long long ws_bytes,
                                  hipStream_t s) {
  if (!pred || !x || !x_out || !next_in || !sqrt_acp || !sqrt_1m || B <= 0 || B > 32767 || HW <= 0) return OTAMD_EINVAL;
  if (n_table <= 0 || t < 0 || t >= n_table || t_prev < 0 || t_prev >= n_table) return OTAMD_EINVAL;
  if (!(cfg_rescale >= 0.f) || !(cfg_scale == cfg_scale)) return OTAMD_EINVAL;
  if (((uintptr_t)pred | (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)next_in) & 15) return OTAMD_EINVAL;
  const long long nblk = (HW + STEP_THREADS - 1) / STEP_THREADS;
  if (nblk > 0x7fffffffll) return OTAMD_EINVAL;
  const bool rescale = cfg_rescale > 0.f;
  if (rescale && (!ws || ((uintptr_t)ws & 7) || ws_bytes < otamd_cfg_ddim_step_ws_bytes(B, HW))) return OTAMD_EINVAL;
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (rescale) {
    cfg_stats_kernel<<<grid, STEP_THREADS, 0, s>>>((const bf16_t*)pred, B, HW, cfg_scale, (double*)ws, (int)nblk);
    OTAMD_CHECK_LAUNCH();
  }
  cfg_ddim_update_kernel<<<grid, STEP_THREADS, 0, s>>>((const bf16_t*)pred, x, x_out, (bf16_t*)next_in, B, HW,
                                                       cfg_scale, cfg_rescale, v_pred ? 1 : 0, sqrt_acp, sqrt_1m, t,
                                                       t_prev, rescale ? (const double*)ws : nullptr, (int)nblk);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

OTAMD_API int otamd_nhwc_to_rgb8(const void* x, int cpad, long long npix, void* out, hipStream_t s) {
  if (!x || !out || npix <= 0 || cpad < 3) return OTAMD_EINVAL;
  if (cpad == 8 && ((uintptr_t)x & 15)) return OTAMD_EINVAL;
  if ((uintptr_t)out & 3) return OTAMD_EINVAL;
  const long long groups = (npix + 3) / 4;
  const long long blocks = (groups + 255) / 256;
  if (blocks > 0x7fffffffll) return OTAMD_EINVAL;
  nhwc_to_rgb8_kernel<<<(unsigned)blocks, 256, 0, s>>>((const bf16_t*)x, cpad, npix, (uint8_t*)out);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
