// AttnArgs (include/otamd.h's layout), the host-side launcher and range check shared by attention.hip,
// attention_wide.hip and attention_vae.hip, and the entry points of attention_wide.hip that attention.hip dispatches to.
#pragma once
#include <cstddef>
#include <mutex>
#include <unordered_set>
#include "common.h"

struct AttnArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o; float* lse;
  const bf16_t* dout; const float* delta; bf16_t* dq; bf16_t* dk; bf16_t* dv; float* dk32; float* dv32;
  long long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;     // token strides (elements)
  long long bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv;     // batch strides (elements)
  int B, H, Nq, Nk, Dv;
  float scale;
  int qsplit;
  int xcd;   // (the header's reserved pad_; callers pass 0) set by the launchers: XCD-grouped block order
};
static_assert(sizeof(AttnArgs) == 256 && offsetof(AttnArgs, ldq) == 96 && offsetof(AttnArgs, B) == 224,
              "AttnArgs must keep the layout of include/otamd.h");

// 256 threads, lds_bytes of dynamic LDS; the opt-in above 64 KiB is made once per kernel (its LDS size is fixed)
inline void attn_launch(void (*kern)(AttnArgs), dim3 grid, int lds_bytes, hipStream_t stream, const AttnArgs& a) {
  {
    static std::mutex mu;
    static std::unordered_set<const void*> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.insert((const void*)kern).second)
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, stream, a);
}

// the per-(batch, head) DMA descriptors address rows of `width` columns with 31-bit byte offsets
inline bool fits31(int rows, long long ld, int width) { return ((long long)rows * ld + width) * 2 < 0x7fff0000LL; }

// heads of 129..160 columns (attention_wide.hip); arguments already checked by otamd_attn_fwd / otamd_attn_bwd
int otamd_attn_wide_fwd(const AttnArgs& a, hipStream_t stream);
int otamd_attn_wide_bwd(const AttnArgs& a, float* ws, hipStream_t stream);
long long otamd_attn_wide_ws_bytes(const AttnArgs& a);
