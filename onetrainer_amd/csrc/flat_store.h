// What every optimizer kernel file over the flat parameter store shares (adamw.hip, adafactor.hip, came.hip,
// prodigy.hip, schedule_free.hip, adamw8bit.hip, ema.hip), each written once:
//   device  fs_load8 / fs_load1 / fs_store8   16-byte vectors at an 8-aligned element index, partial ones masked
//           fs_clip                           the pending global-norm clip on one gradient element
//           fs_write_params                   the parameter write of the three store forms
//           fs_find_group, fs_valid           the group of a vector and its lanes inside that group
//           fs_seed_key                       the 32-bit stochastic-rounding key of a 64-bit seed
//           NormChunk                         the chunk table of the global grad norm
//   host    fs_grid                           workgroups of a launch under the OTAMD_ADAMW_BLOCKS cap
//           fs_window_ok, fs_groups_ok, fs_form_ok, fs_aligned16   the checks of a C entry point
//           fs_groups_arg                     the group structs as the kernel's by-value argument
//           fs_dispatch                       one kernel instantiation per store form
// Store forms (`form` of the C ABI, FORM of the kernels): 0 a bf16 store with bf16 gradients; 1 an fp32 store with fp32
// gradients; 2 the fp32 master with bf16 gradients and the bf16 working copy W = rne(master).  ema.hip's form codes
// mean something else (shadow against parameter dtype) and stay its own.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#define FS_MAX_GROUPS 8   // parameter groups of one launch: the by-value group argument of every kernel

// the chunk table of the global grad norm: (element begin, element end, tensor index) per workgroup; begin is a
// multiple of 8, a chunk never crosses a tensor
struct NormChunk { long long begin, end; int tensor; int pad; };

// eight elements at an 8-aligned element index
template <typename T> __device__ __forceinline__ void fs_load8(const T* base, long long e, float* f);
template <> __device__ __forceinline__ void fs_load8<bf16_t>(const bf16_t* base, long long e, float* f) {
  const bf8 v = *reinterpret_cast<const bf8*>(base + e);
  unpack8(v, f);
}
template <> __device__ __forceinline__ void fs_load8<float>(const float* base, long long e, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(base + e);
  const float4 b = *reinterpret_cast<const float4*>(base + e + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <typename T> __device__ __forceinline__ float fs_load1(const T* base, long long e);
template <> __device__ __forceinline__ float fs_load1<bf16_t>(const bf16_t* base, long long e) { return bf2f(base[e]); }
template <> __device__ __forceinline__ float fs_load1<float>(const float* base, long long e) { return base[e]; }

// the pending global-norm clip on one gradient element, rounded as the AdamW kernels round it
template <bool BFROUND> __device__ __forceinline__ float fs_clip(float g, float coef, bool clip) {
  if (!clip) return g;
  return BFROUND ? rbf(g * coef) : g * coef;
}

// eight values at an 8-aligned element index; partial vectors element-wise (neighbours never write the same bytes)
__device__ __forceinline__ void fs_store8(float* base, long long v, const float* x, unsigned valid) {
  if (valid == 0xFFu) {
    *reinterpret_cast<float4*>(base + v) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(base + v + 4) = make_float4(x[4], x[5], x[6], x[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (valid >> j & 1) base[v + j] = x[j];
  }
}
__device__ __forceinline__ void fs_store8(bf16_t* base, long long v, const float* x, unsigned valid) {
  if (valid == 0xFFu) {
    *reinterpret_cast<bf8*>(base + v) = pack8(x);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (valid >> j & 1) base[v + j] = f2bf(x[j]);
  }
}

// the stochastic-rounding key of sr_bits (common.h) from the optimizer's 64-bit seed
__device__ __forceinline__ uint32_t fs_seed_key(unsigned long long seed) { return (uint32_t)(seed ^ (seed >> 32)); }

// ---- the parameter write of an apply kernel -----------------------------------------------------------------------
// FORM 0: x rounded here (stochastic bits of key k at the store index, or RNE); 1: fp32; 2: fp32 master + W
template <int FORM, typename TP>
__device__ __forceinline__ void fs_write_params(TP* P, bf16_t* W, long long v, float* x, unsigned valid, int sr,
                                                uint32_t k) {
  if constexpr (FORM == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      x[j] = sr ? __uint_as_float((__float_as_uint(x[j]) + sr_bits(k, (uint64_t)(v + j))) & 0xFFFF0000u) : rbf(x[j]);
  }
  fs_store8(P, v, x, valid);
  if constexpr (FORM == 2) fs_store8(W, v, x, valid);
}

// ---- parameter groups: sorted element ranges [begin, end) in a struct { G g[FS_MAX_GROUPS]; int n; } --------------
// the last group that begins at or before element e
template <typename Groups>
__device__ __forceinline__ int fs_find_group(const Groups& G, long long e) {
  int gi = 0;
#pragma unroll
  for (int i = 1; i < FS_MAX_GROUPS; ++i)
    if (i < G.n && e >= G.g[i].begin) gi = i;
  return gi;
}

// lanes of the vector at e0 that belong to [begin, end) (tensors start on vectors, so begin <= e0 for the group
// fs_find_group returns; the mask keeps the store's padding, which belongs to no group, untouched)
__device__ __forceinline__ unsigned fs_valid(long long e0, long long begin, long long end) {
  if (e0 < begin || e0 >= end) return 0u;
  return e0 + 8 <= end ? 0xFFu : (1u << (int)(end - e0)) - 1u;
}

// ---- host: what the C entry points share ---------------------------------------------------------------------------
// workgroups for `units` of work at `per_block` a workgroup: at most dflt, at most OTAMD_ADAMW_BLOCKS when that is
// set (read once per translation unit), at least 1.  An update overlapped with the next forward on its own stream
// (util/optimizer/adamw_fused.py) holds only that many CUs' worth of slots.
static inline int fs_grid(long long units, int per_block, long long dflt) {
  static const long long cap = [] {
    const char* e = getenv("OTAMD_ADAMW_BLOCKS");
    return e ? atoll(e) : 0LL;
  }();
  const long long most = cap > 0 ? std::min(cap, dflt) : dflt;
  return (int)std::max(1LL, std::min((units + per_block - 1) / per_block, most));
}

// [begin, end): a launch window of whole vectors; inside a store of n elements (a multiple of 8)
static inline bool fs_window_ok(long long begin, long long end) {
  return begin >= 0 && begin <= end && (begin % 8) == 0 && (end % 8) == 0;
}
static inline bool fs_window_ok(long long n, long long begin, long long end) {
  return n >= 0 && (n % 8) == 0 && end <= n && fs_window_ok(begin, end);
}

static inline bool fs_group_count_ok(int n_groups) { return n_groups >= 1 && n_groups <= FS_MAX_GROUPS; }

// groups sorted by begin, disjoint, inside [0, n), begin on a vector
template <typename G>
static bool fs_groups_ok(const G* groups, int n_groups, long long n) {
  if (!groups || !fs_group_count_ok(n_groups)) return false;
  long long prev = 0;
  for (int i = 0; i < n_groups; ++i) {
    if (groups[i].begin < prev || groups[i].end < groups[i].begin || groups[i].end > n || (groups[i].begin % 8) != 0)
      return false;
    prev = groups[i].end;
  }
  return true;
}

static inline bool fs_form_ok(int form, const void* w16) { return form >= 0 && form <= 2 && (form != 2 || w16); }

// every pointer on 16 bytes (null pointers pass: the caller checks which may be null)
template <typename... P>
static bool fs_aligned16(const P*... p) {
  return (((uintptr_t)p | ... | (uintptr_t)0) & 15) == 0;
}

// the first n_groups structs into the kernel's by-value argument GS { G g[FS_MAX_GROUPS]; [int n;] }
template <typename GS>
static auto fs_set_n(GS& out, int n, int) -> decltype((void)out.n) { out.n = n; }
template <typename GS>
static void fs_set_n(GS&, int, long) {}
template <typename GS, typename G>
static GS fs_groups_arg(const G* groups, int n_groups) {
  GS out = {};
  for (int i = 0; i < n_groups; ++i) out.g[i] = groups[i];
  fs_set_n(out, n_groups, 0);
  return out;
}

// one store form as a type: the element types of the parameters and the gradients, the stochastic-rounding flag
// (bf16 stores only) and the working copy (master stores only) a launch passes on
template <int FORM> struct FsForm {
  static constexpr int form = FORM;
  using TP = std::conditional_t<FORM == 0, bf16_t, float>;
  using TG = std::conditional_t<FORM == 1, float, bf16_t>;
  static int sr(int stochastic_rounding) { return FORM == 0 ? stochastic_rounding : 0; }
  static bf16_t* w(void* w16) { return FORM == 2 ? (bf16_t*)w16 : nullptr; }
};
// f(FsForm<form>{}) for a form that fs_form_ok accepted
template <typename F>
static auto fs_dispatch(int form, F&& f) {
  if (form == 0) return f(FsForm<0>{});
  if (form == 1) return f(FsForm<1>{});
  return f(FsForm<2>{});
}
