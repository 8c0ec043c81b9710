// Exponential moving average of the trained weights over a flat parameter store.  Replaces, per parameter tensor,
// the reference's
//   modules/module/EMAModule.py:37-54  (EMAModuleWrapper.step: ema.add_(one_minus_decay * (parameter - ema)))
// with ONE launch over an element range of the flat buffers (the reference runs three torch ops per tensor in a
// Python loop).
//
// Numerics: each of the three torch ops (sub, scalar mul, add_) rounds to its result dtype, in that order; the
// scalar is Python's double 1 - decay narrowed to fp32, as torch applies a Python scalar to a float / bf16 tensor.
// Compile with -ffp-contract=off so the multiply and the add stay two roundings.  No reductions, no reassociation:
// the result is bit-identical to the reference's (tests/test_ema_gpu.py against tests/golden/ema_steps.npz).
//
// Forms (shadow e, parameters p):
//   0  bf16 / bf16   rbf(e + rbf(omd * rbf(p - e)))                        6 B per element
//   1  fp32 / fp32   e + omd * (p - e), three fp32 roundings               12 B per element
//   2  fp32 / bf16   as 1 with p widened exactly (torch's type promotion)  10 B per element
// A pure streaming pass: 16-byte accesses of the shadow, a grid-stride loop with the next granules' loads in flight,
// non-temporal accesses for the shadow (touched once per update); the parameters are read with the default policy,
// the optimizer has just written them and the next forward reads them.  The kernels need no group table and run over
// the store's padding too: padding is 0 in both buffers and 0 + omd * (0 - 0) stays 0.
#include "flat_store.h"

// 1024-thread workgroups, two per CU (256 CUs), a grid-stride loop over the rest, two granules per thread and sweep.
// Measured on MI355X over 2.567 G elements, hipEvents, median of 10 (the fused AdamW's 14 B per element in the same
// run: 6.24 ms, 5.76 TB/s):
//   bf16 2.81 ms (5.48 TB/s), fp32 5.90 ms (5.22 TB/s), fp32 shadow of bf16 5.47 ms (4.69 TB/s).
// Tried: 256-thread workgroups x 2048 with one granule per thread, 3.3 / 6.5 ms; four granules, non-temporal
// parameter loads, twice the threads: each within 2 %.  Form 2 with a thread on 8 elements (32 bytes of shadow at a
// 32-byte lane stride, two half-used lines per wave access) took 7.9 ms; hence its 4-element units with 8-byte
// parameter loads.
#define EMA_BLOCK 1024
#define EMA_GRID_CAP 512
#define EMA_UNROLL 2

typedef uint32_t ema_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf8 ema_ld_nt(const bf16_t* base, long long i) {
  const ema_u4 x = __builtin_nontemporal_load(reinterpret_cast<const ema_u4*>(base) + i);
  bf8 r; r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w;
  return r;
}
__device__ __forceinline__ void ema_st_nt(bf16_t* base, long long i, bf8 x) {
  ema_u4 y; y.x = x.w[0]; y.y = x.w[1]; y.z = x.w[2]; y.w = x.w[3];
  __builtin_nontemporal_store(y, reinterpret_cast<ema_u4*>(base) + i);
}
__device__ __forceinline__ float4v ema_ld_nt(const float* base, long long i) {
  return __builtin_nontemporal_load(reinterpret_cast<const float4v*>(base) + i);
}
__device__ __forceinline__ void ema_st_nt(float* base, long long i, float4v x) {
  __builtin_nontemporal_store(x, reinterpret_cast<float4v*>(base) + i);
}

// one element, fp32 shadow: parameter - ema, one_minus_decay * that, ema.add_(that)
__device__ __forceinline__ float ema_elem_f32(float e, float p, float omd) {
  float d = p - e;
  d = omd * d;
  return e + d;
}
// one element, bf16 shadow: every op's result is a bf16 tensor
__device__ __forceinline__ float ema_elem_bf16(float e, float p, float omd) {
  float d = rbf(p - e);
  d = rbf(omd * d);
  return rbf(e + d);
}

// form 0.  [v0, v1): 16-byte granules (8 bf16) of both buffers; a thread takes granules i + u T of a sweep of
// EMA_UNROLL T granules (T threads in the grid), so every wave access is 1 KiB contiguous
__global__ void __launch_bounds__(EMA_BLOCK) ema_bf16_kernel(bf16_t* __restrict__ E, const bf16_t* __restrict__ P,
                                                             long long v0, long long v1, float omd) {
  constexpr int U = EMA_UNROLL;
  const long long T = (long long)gridDim.x * EMA_BLOCK;
  long long i = v0 + blockIdx.x * (long long)EMA_BLOCK + threadIdx.x;
  const bf8* P8 = reinterpret_cast<const bf8*>(P);
  // software pipeline: the next sweep's loads are in flight while this one is computed
  bf8 ev[U], pv[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (i + u * T < v1) { ev[u] = ema_ld_nt(E, i + u * T); pv[u] = P8[i + u * T]; }
  for (; i < v1; i += U * T) {
    const long long in = i + U * T;
    bf8 en[U], pn[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (in + u * T < v1) { en[u] = ema_ld_nt(E, in + u * T); pn[u] = P8[in + u * T]; }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * T < v1) {
        float e[8], p[8];
        unpack8(ev[u], e); unpack8(pv[u], p);
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = ema_elem_bf16(e[j], p[j], omd);
        ema_st_nt(E, i + u * T, pack8(e));
      }
#pragma unroll
    for (int u = 0; u < U; ++u) { ev[u] = en[u]; pv[u] = pn[u]; }
  }
}

__device__ __forceinline__ float4v ema_vec_f32(float4v e, float4v p, float omd) {
  float4v r;
  r.x = ema_elem_f32(e.x, p.x, omd); r.y = ema_elem_f32(e.y, p.y, omd);
  r.z = ema_elem_f32(e.z, p.z, omd); r.w = ema_elem_f32(e.w, p.w, omd);
  return r;
}

// 4 parameters of unit q as floats: a 16-byte granule of an fp32 store, an 8-byte one of a bf16 store (widened exactly)
__device__ __forceinline__ float4v ema_ld_p4(const float* P, long long q) {
  return reinterpret_cast<const float4v*>(P)[q];
}
__device__ __forceinline__ float4v ema_ld_p4(const bf16_t* P, long long q) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const u2 x = reinterpret_cast<const u2*>(P)[q];
  float4v r;
  r.x = __uint_as_float(x.x << 16); r.y = __uint_as_float(x.x & 0xffff0000u);
  r.z = __uint_as_float(x.y << 16); r.w = __uint_as_float(x.y & 0xffff0000u);
  return r;
}

// forms 1 (PT float) and 2 (PT bf16_t).  [q0, q1): units of 4 elements, a 16-byte granule of the shadow each;
// a thread takes units i + u T of a sweep, as above
template <typename PT>
__global__ void __launch_bounds__(EMA_BLOCK) ema_f32_kernel(float* __restrict__ E, const PT* __restrict__ P,
                                                            long long q0, long long q1, float omd) {
  constexpr int U = EMA_UNROLL;
  const long long T = (long long)gridDim.x * EMA_BLOCK;
  long long i = q0 + blockIdx.x * (long long)EMA_BLOCK + threadIdx.x;
  float4v ev[U], pv[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (i + u * T < q1) { ev[u] = ema_ld_nt(E, i + u * T); pv[u] = ema_ld_p4(P, i + u * T); }
  for (; i < q1; i += U * T) {
    const long long in = i + U * T;
    float4v en[U], pn[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (in + u * T < q1) { en[u] = ema_ld_nt(E, in + u * T); pn[u] = ema_ld_p4(P, in + u * T); }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * T < q1) ema_st_nt(E, i + u * T, ema_vec_f32(ev[u], pv[u], omd));
#pragma unroll
    for (int u = 0; u < U; ++u) { ev[u] = en[u]; pv[u] = pn[u]; }
  }
}

// ---- C ABI ----------------------------------------------------------------------
// elements per unit of a form's kernel (one thread, one access of the shadow)
static int ema_unit(int form) { return form == 0 ? 8 : 4; }

// elements one full grid covers in one sweep of its grid-stride loop
OTAMD_API int otamd_ema_sweep_elems(int form) {
  if (form < 0 || form > 2) return 0;
  return EMA_GRID_CAP * EMA_BLOCK * EMA_UNROLL * ema_unit(form);
}

// ema, p: flat buffers of the same layout; [begin, end): element range (multiples of 8); form 0 / 1 / 2 as above
OTAMD_API int otamd_ema_range(void* ema, const void* p, int form, long long begin, long long end,
                              float one_minus_decay, hipStream_t stream) {
  if (!ema || !p || form < 0 || form > 2 || !fs_window_ok(begin, end)) return OTAMD_EINVAL;
  if (!fs_aligned16(ema, p)) return OTAMD_EINVAL;
  if (end == begin) return OTAMD_OK;
  const long long u0 = begin / ema_unit(form), u1 = end / ema_unit(form);
  const long long threads = (u1 - u0 + EMA_UNROLL - 1) / EMA_UNROLL;
  const int blocks = (int)std::min<long long>((threads + EMA_BLOCK - 1) / EMA_BLOCK, EMA_GRID_CAP);
  if (form == 0)
    ema_bf16_kernel<<<blocks, EMA_BLOCK, 0, stream>>>((bf16_t*)ema, (const bf16_t*)p, u0, u1, one_minus_decay);
  else if (form == 1)
    ema_f32_kernel<float><<<blocks, EMA_BLOCK, 0, stream>>>((float*)ema, (const float*)p, u0, u1, one_minus_decay);
  else
    ema_f32_kernel<bf16_t><<<blocks, EMA_BLOCK, 0, stream>>>((float*)ema, (const bf16_t*)p, u0, u1, one_minus_decay);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
