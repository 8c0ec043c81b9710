// Concept image augmentations on the device: crop (jitter), flip, rotate, brightness, contrast, saturation, hue.
// Replaces, between the reference's ScaleCropImage and EncodeVAE (modules/dataLoader/mixin/
// DataLoaderText2ImageMixin.py:186-212), the mgds modules RandomFlip, RandomRotate, RandomBrightness,
// RandomContrast, RandomSaturation and RandomHue, and the crop of ScaleCropImage.  One image is scaled on the host
// and uploaded once; every cached variation of it is made here and goes straight into the VAE encoder.
//
// The launch is table-driven (AugEntry per (sample, variation); a mask is a one-channel entry with its image's
// geometry).  Sources differ in Hs x Ws (scale-to-cover leaves one side longer), the outputs of one launch share H x W.
//
//   launch 1  crop at (y0, x0) + flip + rotate as one gather, then brightness; the gray sum of the workgroup's pixels
//             goes to partials[entry][workgroup] when the entry has a contrast factor
//   launch 2  m = (sum of the entry's partials) / (H W); contrast, saturation, hue in place.  Skipped when no entry
//             of the table has a colour factor.
// A stage whose factor is neutral (1, 1, 1, 0; no rotation: cos a == 1 and sin a == 0) is not run, so a crop-only or
// flip-only entry is a bit-exact copy.  The mean is the only cross-pixel dependency: a thread adds its pixels in a
// fixed order, block_sum is a fixed tree, and every workgroup of launch 2 adds the partials in the same fixed order
// (thread t takes t, t + 256, ... ascending, then block_sum).  No atomics: two runs give the same bits.
//
// A workgroup owns a tile of 256 x 16 output pixels: a lane owns 4 consecutive pixels of a row (one 16-byte access
// where the entry's alignment allows, 4 dword accesses with a bounds check otherwise), a wave one 1 KiB row segment,
// and walks 4 rows.  The tile comes from the 3-D grid, so no index is divided anywhere.  Compiled with
// -ffp-contract=off: the operation order below is the one tests/_oracle_augment.py restates.
#include "common.h"

#include <cmath>

#define AUG_QUADS 64   // lanes across a row, 4 pixels each
#define AUG_TW 256     // tile width in pixels
#define AUG_TH 16      // tile rows: 4 waves x 4 rows

struct AugEntry {
  long long src_off;   // the source plane [C][Hs][Ws], elements into the flat fp32 source buffer
  long long out_off;   // the output [C][H][W], elements into the fp32 output buffer
  int C, Hs, Ws;       // C = 3 (image) or 1 (mask)
  int y0, x0;          // top-left of the crop in the source
  int H, W;            // crop = output size
  int flip;            // mirror x within the crop
  float cos_a, sin_a;  // rotation about the crop's centre, positive angle counter-clockwise
  float brightness, contrast, saturation, hue;   // neutral: 1, 1, 1, 0
};

__device__ __forceinline__ float aug_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float aug_gray(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
__device__ __forceinline__ bool aug_has_colour(const AugEntry& e) {
  return e.C == 3 && (e.contrast != 1.f || e.saturation != 1.f || e.hue != 0.f);
}

// one crop pixel (y, x): 0 outside the crop, also where the source has pixels there (the reference rotates the crop)
__device__ __forceinline__ float aug_tap(const float* __restrict__ p, const AugEntry& e, int y, int x) {
  if ((unsigned)y >= (unsigned)e.H || (unsigned)x >= (unsigned)e.W) return 0.f;
  const int sx = e.flip ? e.W - 1 - x : x;
  return p[(long long)(e.y0 + y) * e.Ws + e.x0 + sx];
}

__global__ void __launch_bounds__(256) image_augment_geometry_kernel(const AugEntry* __restrict__ tab,
                                                                     const float* __restrict__ src,
                                                                     float* __restrict__ out,
                                                                     float* __restrict__ partials) {
  __shared__ float red[4];
  const AugEntry e = tab[blockIdx.z];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j0 = (blockIdx.x * AUG_QUADS + lane) * 4;
  const long long splane = (long long)e.Hs * e.Ws, oplane = (long long)e.H * e.W;
  const float* s = src + e.src_off;
  float* o = out + e.out_off;
  const bool identity = e.cos_a == 1.f && e.sin_a == 0.f;
  const bool vec_out = !(e.W & 3) && !(e.out_off & 3);
  const bool vec_in = identity && vec_out && !(e.Ws & 3) && !(e.src_off & 3) && !(e.x0 & 3);
  const bool bright = e.brightness != 1.f;
  const bool want_mean = e.C == 3 && e.contrast != 1.f;
  const float cx = (float)(e.W - 1) * 0.5f, cy = (float)(e.H - 1) * 0.5f;
  float gsum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = blockIdx.y * AUG_TH + wv + 4 * r;
    if (i >= e.H || j0 >= e.W) continue;
    const int nk = min(4, e.W - j0);   // < 4 only in the last quad of a width that is no multiple of 4
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= e.C) break;
      const float* p = s + c * splane;
      if (identity) {
        const float* row = p + (long long)(e.y0 + i) * e.Ws + e.x0;
        if (vec_in) {
          if (!e.flip) {
            const float4v t = *reinterpret_cast<const float4v*>(row + j0);
            v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
          } else {
            const float4v t = *reinterpret_cast<const float4v*>(row + (e.W - 4 - j0));
            v[c][0] = t.w; v[c][1] = t.z; v[c][2] = t.y; v[c][3] = t.x;
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nk) v[c][k] = row[e.flip ? e.W - 1 - (j0 + k) : j0 + k];
        }
      } else {
        const float yo = (float)i - cy;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k >= nk) break;
          const float xo = (float)(j0 + k) - cx;
          const float xs = (e.cos_a * xo - e.sin_a * yo) + cx;
          const float ys = (e.sin_a * xo + e.cos_a * yo) + cy;
          const float fx = floorf(xs), fy = floorf(ys);
          const float ax = xs - fx, ay = ys - fy;
          const int ix = (int)fx, iy = (int)fy;
          const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
          v[c][k] = ((w00 * aug_tap(p, e, iy, ix) + w01 * aug_tap(p, e, iy, ix + 1)) +
                     w10 * aug_tap(p, e, iy + 1, ix)) + w11 * aug_tap(p, e, iy + 1, ix + 1);
        }
      }
      if (bright) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nk) v[c][k] = aug_clamp01(v[c][k] * e.brightness);
      }
    }
    if (want_mean) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nk) gsum += aug_gray(v[0][k], v[1][k], v[2][k]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= e.C) break;
      float* q = o + c * oplane + (long long)i * e.W + j0;
      if (vec_out) {
        const float4v t = {v[c][0], v[c][1], v[c][2], v[c][3]};
        *reinterpret_cast<float4v*>(q) = t;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nk) q[k] = v[c][k];
      }
    }
  }
  if (want_mean) {   // uniform over the workgroup
    const float t = block_sum(gsum, red);
    if (threadIdx.x == 0)
      partials[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
  }
}

// hue: RGB -> HSV (v = max, s = (max - min) / max, the sextant h; h = 0 on a gray pixel), h <- (h + f) mod 1, back
__device__ __forceinline__ void aug_hue(float& r, float& g, float& b, float f) {
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float d = mx - mn;
  if (d == 0.f) return;   // gray (black included): s = 0, the pixel keeps its value
  const float sat = d / mx;
  float h;
  if (r == mx) h = (g - b) / d;
  else if (g == mx) h = 2.f + (b - r) / d;
  else h = 4.f + (r - g) / d;
  h = h / 6.f + f;
  h = h - floorf(h);
  const float h6 = h * 6.f;
  const float fi = floorf(h6);
  const float fr = h6 - fi;
  const float p = mx * (1.f - sat), q = mx * (1.f - sat * fr), t = mx * (1.f - sat * (1.f - fr));
  const int i = (int)fi;   // 0..6; 6 (h rounded up to 1) is sextant 0 with fr = 0
  if (i == 0 || i == 6) { r = mx; g = t; b = p; }
  else if (i == 1) { r = q; g = mx; b = p; }
  else if (i == 2) { r = p; g = mx; b = t; }
  else if (i == 3) { r = p; g = q; b = mx; }
  else if (i == 4) { r = t; g = p; b = mx; }
  else { r = mx; g = p; b = q; }
}

__global__ void __launch_bounds__(256) image_augment_colour_kernel(const AugEntry* __restrict__ tab,
                                                                   float* __restrict__ out,
                                                                   const float* __restrict__ partials) {
  __shared__ float red[4];
  const AugEntry e = tab[blockIdx.z];
  if (!aug_has_colour(e)) return;   // uniform over the workgroup
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j0 = (blockIdx.x * AUG_QUADS + lane) * 4;
  const long long oplane = (long long)e.H * e.W;
  float* o = out + e.out_off;
  const bool vec = !(e.W & 3) && !(e.out_off & 3);
  const bool cont = e.contrast != 1.f, sat = e.saturation != 1.f, hue = e.hue != 0.f;
  float cm = 0.f;
  if (cont) {
    const int tiles = gridDim.x * gridDim.y;
    const float* part = partials + (long long)blockIdx.z * tiles;
    float t = 0.f;
    for (int k = threadIdx.x; k < tiles; k += 256) t += part[k];
    const float m = block_sum(t, red) / (float)oplane;
    cm = (1.f - e.contrast) * m;
  }
  const float s1 = 1.f - e.saturation;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = blockIdx.y * AUG_TH + wv + 4 * r;
    if (i >= e.H || j0 >= e.W) continue;
    const int nk = min(4, e.W - j0);
    float* q = o + (long long)i * e.W + j0;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec) {
        const float4v t = *reinterpret_cast<const float4v*>(q + c * oplane);
        v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nk) v[c][k] = q[c * oplane + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= nk) break;
      float rr = v[0][k], gg = v[1][k], bb = v[2][k];
      if (cont) {
        rr = aug_clamp01(e.contrast * rr + cm);
        gg = aug_clamp01(e.contrast * gg + cm);
        bb = aug_clamp01(e.contrast * bb + cm);
      }
      if (sat) {
        const float sg = s1 * aug_gray(rr, gg, bb);
        rr = aug_clamp01(e.saturation * rr + sg);
        gg = aug_clamp01(e.saturation * gg + sg);
        bb = aug_clamp01(e.saturation * bb + sg);
      }
      if (hue) aug_hue(rr, gg, bb, e.hue);
      v[0][k] = rr; v[1][k] = gg; v[2][k] = bb;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec) {
        const float4v t = {v[c][0], v[c][1], v[c][2], v[c][3]};
        *reinterpret_cast<float4v*>(q + c * oplane) = t;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nk) q[c * oplane + k] = v[c][k];
      }
    }
  }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_aug_entry_size(void) { return (int)sizeof(AugEntry); }

// floats of the partial-sum workspace of a launch of n entries of H x W (one per workgroup of launch 1)
OTAMD_API long long otamd_image_augment_ws_floats(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0) return 0;
  return (long long)n * ceil_div(H, AUG_TH) * ceil_div(W, AUG_TW);
}

// table_dev / table_host: the same AugEntry[n] on the device and on the host.  Every entry is checked here against
// the buffer sizes before anything is launched: the kernels trust the table.  src: flat fp32 source planes in [0, 1];
// out: fp32, every entry's [C][H][W] at its out_off; ws: otamd_image_augment_ws_floats(n, H, W) floats.
OTAMD_API int otamd_image_augment(const void* table_dev, const void* table_host, int n, int H, int W, const float* src,
                                  long long src_numel, float* out, long long out_numel, float* ws, long long ws_floats,
                                  hipStream_t stream) {
  if (!table_dev || !table_host || n < 0 || n > 65535 || H <= 0 || W <= 0 || !src || !out || !ws) return OTAMD_EINVAL;
  if (((uintptr_t)src | (uintptr_t)out) & 15) return OTAMD_EINVAL;
  if (n == 0) return OTAMD_OK;
  const int tiles_x = ceil_div(W, AUG_TW), tiles_y = ceil_div(H, AUG_TH);
  if (tiles_y > 65535 || (long long)H * W > 0x7fffffffLL) return OTAMD_EINVAL;
  if (ws_floats < (long long)n * tiles_x * tiles_y) return OTAMD_EINVAL;
  const AugEntry* t = (const AugEntry*)table_host;
  bool colour = false;
  for (int i = 0; i < n; ++i) {
    const AugEntry& e = t[i];
    if ((e.C != 1 && e.C != 3) || e.H != H || e.W != W || e.Hs <= 0 || e.Ws <= 0) return OTAMD_EINVAL;
    if ((long long)e.Hs * e.Ws > 0x7fffffffLL) return OTAMD_EINVAL;
    if (e.y0 < 0 || e.x0 < 0 || (long long)e.y0 + H > e.Hs || (long long)e.x0 + W > e.Ws) return OTAMD_EINVAL;
    if (e.src_off < 0 || e.src_off > src_numel || (long long)e.C * e.Hs * e.Ws > src_numel - e.src_off)
      return OTAMD_EINVAL;
    if (e.out_off < 0 || e.out_off > out_numel || (long long)e.C * H * W > out_numel - e.out_off) return OTAMD_EINVAL;
    if (e.flip != 0 && e.flip != 1) return OTAMD_EINVAL;
    const float n2 = e.cos_a * e.cos_a + e.sin_a * e.sin_a;
    if (!(std::fabs(n2 - 1.f) <= 1e-3f)) return OTAMD_EINVAL;   // also refuses NaN
    if (!(e.brightness >= 0.f && e.brightness <= 1e4f) || !(e.contrast >= 0.f && e.contrast <= 1e4f) ||
        !(e.saturation >= 0.f && e.saturation <= 1e4f) || !(e.hue >= -1.f && e.hue <= 1.f))
      return OTAMD_EINVAL;
    colour = colour || (e.C == 3 && (e.contrast != 1.f || e.saturation != 1.f || e.hue != 0.f));
  }
  const dim3 grid(tiles_x, tiles_y, n);
  image_augment_geometry_kernel<<<grid, 256, 0, stream>>>((const AugEntry*)table_dev, src, out, ws);
  if (colour) image_augment_colour_kernel<<<grid, 256, 0, stream>>>((const AugEntry*)table_dev, out, ws);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
