// AttnArgs (include/otamd.h's layout) and the entry points of attention_wide.hip that attention.hip dispatches to.
#pragma once
#include <cstddef>
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

// heads of 129..160 columns (attention_wide.hip); arguments already checked by otamd_attn_fwd / otamd_attn_bwd
int otamd_attn_wide_fwd(const AttnArgs& a, hipStream_t stream);
int otamd_attn_wide_bwd(const AttnArgs& a, float* ws, hipStream_t stream);
long long otamd_attn_wide_ws_bytes(const AttnArgs& a);
