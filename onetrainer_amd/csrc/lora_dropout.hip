// LoRA dropout (LoRAModule.forward, modules/module/LoRAModule.py:319-323: lora_up(dropout(lora_down(x)))), in place on
// the down projection's output t [M, width] (bf16, contiguous), and in the backward on u = dy (sB) with the same mask,
// which is drawn again instead of being stored.
//
// Mask: one Philox4x32-10 call per row and per group of 4 consecutive columns.  Wq = ceil(width / 4);
//   call index q = site_id * 2^40 + (row0 + m) * Wq + quad, counter = (lo32(q), hi32(q), 6, TAG), key = the seed;
//   word k of the call belongs to column 4 * quad + k (words past `width` are unused).
// Keep rule: element kept iff (uint64)word >= thr, thr = floor(p * 2^32) from the host: no float enters the
//   decision; thr = 0 keeps everything, thr = 2^32 nothing.
// Value: kept -> bf16_rne(float(t) * scale), scale = fp32(1 / (1 - p)) from the host; dropped -> +0.
// The seed is read from device memory, so a captured step draws a new mask on every replay; row0 is the row of the
// GLOBAL (all data-parallel ranks) tensor that row 0 of t is, so each rank draws its slice of the global mask.
// The reference draws from torch's device generator, whose stream cannot be reproduced: masks differ by construction.
#include "common.h"
#include "philox.h"

#define LORA_DROP_STREAM 6u
#define LORA_DROP_TAG 0x64726f70u   // "drop"
#define LORA_DROP_MAX_BLOCKS 2048   // 256 CUs x 8 blocks; the rest by grid stride

__device__ __forceinline__ bf16_t drop_one(bf16_t t, uint32_t word, unsigned long long thr, float scale) {
  return (unsigned long long)word >= thr ? f2bf(bf2f(t) * scale) : (bf16_t)0;
}

// RESTART (the validation pass): every sample's rows count from 0, so a sample's mask does not depend on the batch
//   it is in: row m of t is row (m % rows_per) of its sample when the rows are sample-major (rows_per = M / B, the
//   UNet's [B, tokens] rows), row (m / -rows_per) when they are token-major (rows_per = -B, FLUX's r = t * B + b).
// VEC: width % 4 == 0 and t 8-byte aligned, so quad i of the flat [M * Wq] quad index is the 8 bytes at t + 4 i
template <bool VEC, bool RESTART = false>
__global__ void __launch_bounds__(256) lora_dropout_kernel(bf16_t* t, long long nquads, int width, int Wq,
                                                           unsigned long long q0, const unsigned long long* seed_p,
                                                           unsigned long long thr, float scale,
                                                           long long rows_per = 0) {
  const unsigned long long seed = *seed_p;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nquads;
       i += (long long)gridDim.x * blockDim.x) {
    unsigned long long q = q0 + (unsigned long long)i;   // (row0 + m) * Wq + quad = row0 * Wq + i
    if (RESTART) {
      const long long m = i / Wq;
      const long long r = rows_per > 0 ? m % rows_per : m / -rows_per;
      q = q0 + (unsigned long long)(r * Wq + (i - m * Wq));
    }
    const Philox r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), LORA_DROP_STREAM, LORA_DROP_TAG, k0, k1);
    if (VEC) {
      uint2* p = reinterpret_cast<uint2*>(t) + i;
      const uint2 v = *p;
      uint2 o;
      o.x = (uint32_t)drop_one((bf16_t)v.x, r.v[0], thr, scale) |
            ((uint32_t)drop_one((bf16_t)(v.x >> 16), r.v[1], thr, scale) << 16);
      o.y = (uint32_t)drop_one((bf16_t)v.y, r.v[2], thr, scale) |
            ((uint32_t)drop_one((bf16_t)(v.y >> 16), r.v[3], thr, scale) << 16);
      *p = o;
    } else {
      const long long m = i / Wq;
      const int c0 = 4 * (int)(i - m * Wq);
      bf16_t* row = t + m * width;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < width) row[c0 + k] = drop_one(row[c0 + k], r.v[k], thr, scale);
    }
  }
}

// t: bf16 [M, width] contiguous, modified in place; seed: device pointer to the 64-bit seed; thr in [0, 2^32];
// site_id in [0, 2^24); (row0 + M) * ceil(width / 4) <= 2^40
OTAMD_API int otamd_lora_dropout(void* t, long long M, int width, const unsigned long long* seed, int site_id,
                                 long long row0, unsigned long long thr, float scale, hipStream_t s) {
  const long long lim = 1ll << 40;
  if (!t || !seed || M < 0 || width <= 0 || row0 < 0 || M > lim || row0 > lim) return OTAMD_EINVAL;
  if (thr > (1ull << 32) || site_id < 0 || site_id >= (1 << 24) || !(scale >= 0.f)) return OTAMD_EINVAL;
  if (((uintptr_t)t & 1) || ((uintptr_t)seed & 7)) return OTAMD_EINVAL;
  const int Wq = (width + 3) / 4;
  if (row0 + M > lim / Wq) return OTAMD_EINVAL;   // (row0 + M) * Wq > 2^40
  if (M == 0) return OTAMD_OK;
  const long long nquads = M * Wq;
  const unsigned long long q0 = ((unsigned long long)site_id << 40) + (unsigned long long)(row0 * Wq);
  const long long nb = (nquads + 255) / 256;
  const int grid = (int)(nb > LORA_DROP_MAX_BLOCKS ? LORA_DROP_MAX_BLOCKS : nb);
  if (width % 4 == 0 && ((uintptr_t)t & 7) == 0)
    lora_dropout_kernel<true><<<grid, 256, 0, s>>>((bf16_t*)t, nquads, width, Wq, q0, seed, thr, scale);
  else
    lora_dropout_kernel<false><<<grid, 256, 0, s>>>((bf16_t*)t, nquads, width, Wq, q0, seed, thr, scale);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// the same with per-sample row numbering (the validation pass): rows_per > 0 = rows of one sample, sample-major rows
// (M % rows_per == 0); rows_per < 0 = minus the batch size, token-major rows (M % -rows_per == 0)
OTAMD_API int otamd_lora_dropout_per_sample(void* t, long long M, int width, const unsigned long long* seed,
                                            int site_id, long long rows_per, unsigned long long thr, float scale,
                                            hipStream_t s) {
  const long long lim = 1ll << 40;
  if (!t || !seed || M < 0 || width <= 0 || rows_per == 0 || rows_per > lim || rows_per < -lim || M > lim)
    return OTAMD_EINVAL;   // |rows_per| <= 2^40, so the negation below cannot overflow
  if (thr > (1ull << 32) || site_id < 0 || site_id >= (1 << 24) || !(scale >= 0.f)) return OTAMD_EINVAL;
  if (((uintptr_t)t & 1) || ((uintptr_t)seed & 7)) return OTAMD_EINVAL;
  if (M % (rows_per > 0 ? rows_per : -rows_per)) return OTAMD_EINVAL;
  const int Wq = (width + 3) / 4;
  if (M > lim / Wq) return OTAMD_EINVAL;
  if (M == 0) return OTAMD_OK;
  const long long nquads = M * Wq;
  const unsigned long long q0 = (unsigned long long)site_id << 40;
  const long long nb = (nquads + 255) / 256;
  const int grid = (int)(nb > LORA_DROP_MAX_BLOCKS ? LORA_DROP_MAX_BLOCKS : nb);
  if (width % 4 == 0 && ((uintptr_t)t & 7) == 0)
    lora_dropout_kernel<true, true><<<grid, 256, 0, s>>>((bf16_t*)t, nquads, width, Wq, q0, seed, thr, scale, rows_per);
  else
    lora_dropout_kernel<false, true><<<grid, 256, 0, s>>>((bf16_t*)t, nquads, width, Wq, q0, seed, thr, scale,
                                                          rows_per);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
