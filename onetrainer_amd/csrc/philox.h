// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator
// of every device draw of this library.  Counter = (index lo, index hi, stream id, tag), key = the 64-bit seed.
// Stream ids in use: 1 noise, 2 timestep uniform, 3 timestep normal, 4 offset noise, 5 perturbation noise
// (diffusion.hip), 6 LoRA dropout (lora_dropout.hip), 7 the initial latent of a training sample
// (modelSampler/StableDiffusionSampler.py, keyed by the sample's seed), 8 mask removal of the inpainting models
// (inpaint.hip).
#pragma once
#include "common.h"

struct Philox { uint32_t v[4]; };
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Philox o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}
// uniform in (0, 1): 24 random bits, centred
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }
