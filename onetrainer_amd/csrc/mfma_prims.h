// MFMA / LDS-DMA primitives of the gfx950 ring kernels: the one definition shared by attention.hip,
// attention_wide.hip, attention_vae.hip and gemm2_kernel.h.  Device-side, stateless, all __forceinline__; the
// geometry of a kernel (image swizzles, pitches, ring depth) stays in its own file.  A new head width starts here.
#pragma once
#include "common.h"

constexpr float RESCALE_T = 8.0f;   // forward softmax: lazy-max threshold (log2 units)
constexpr float LOG2E = 1.4426950408889634f;
// a buffer offset the descriptor's range check refuses: the lane's bytes arrive as zeros
#ifndef OFF_INVALID   // (gemm2_stage.h, plain C++ that a CPU test compiles too, has the same value as a macro)
constexpr unsigned OFF_INVALID = 0x80000000u;
#endif

typedef __attribute__((address_space(3))) short4v lds_s4;
typedef __attribute__((address_space(3))) void lds_void_t;

#define MEMBAR() asm volatile("" ::: "memory")
#define WAIT_LDS() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define WAIT_VM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define BARRIER()                 \
  do {                            \
    MEMBAR();                     \
    __builtin_amdgcn_s_barrier(); \
    MEMBAR();                     \
  } while (0)
// gfx950's s_barrier waits for none of this wave's outstanding ds_reads or ds_writes (cdna_hip_programming.md §5), so
// the barrier that guards an LDS slot drains lgkmcnt first.  Writes: s_barrier alone does not publish them.  Reads: the
// compiler sinks the last MFMA of a tile (with the lgkmcnt wait for its operand reads) below a raw s_barrier, and
// another wave's refill DMA then races the reads this wave had issued (dQ run-to-run differences under LDS
// contention from co-resident kernels, round 6).  tests/test_lds_barriers.py checks the shipped assembly for it.
#define BARRIER_LDS()             \
  do {                            \
    WAIT_LDS();                   \
    __builtin_amdgcn_s_barrier(); \
    MEMBAR();                     \
  } while (0)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS-DMA, 16 / 4 bytes per lane (1 KiB / 256 B per wave instruction): 64 lanes from rs[off] to lds[16 lane ..].
// Inline asm on purpose: the compiler's waitcnt pass cannot prove that a later ds_read of ANOTHER LDS stage does not
// alias an in-flight builtin LDS-DMA and would drain vmcnt in front of it, serialising the ring.  Ordering is owned
// by the caller: every read of a stage follows a vmcnt wait + barrier on its DMA.
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, char* lds, unsigned off) {
  const unsigned m0 = (unsigned)(size_t)(lds_void_t*)lds;
  asm volatile("buffer_load_dwordx4 %1, %2, 0 offen lds" ::"{m0}"(m0), "v"(off), "s"(rs) : "memory");
}
__device__ __forceinline__ void dma4(__amdgpu_buffer_rsrc_t rs, char* lds, unsigned off) {
  const unsigned m0 = (unsigned)(size_t)(lds_void_t*)lds;
  asm volatile("buffer_load_dword %1, %2, 0 offen lds" ::"{m0}"(m0), "v"(off), "s"(rs) : "memory");
}
// from rs[voff + soff], soff wave-uniform (a scalar register); the range check sees voff alone
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, char* lds, unsigned voff, unsigned soff) {
  const unsigned m0 = (unsigned)(size_t)(lds_void_t*)lds;
  asm volatile("buffer_load_dwordx4 %1, %2, %3 offen lds" ::"{m0}"(m0), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// raw buffer descriptor of `bytes` bytes at base: lanes past the end read zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, long long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ float16v mfma32(const bf16x8& a, const bf16x8& b, const float16v& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float16v zero16() {
  float16v z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// accumulator registers 8s .. 8s+7 as the next MFMA's B operand (k = the accumulator's row)
__device__ __forceinline__ bf16x8 pack_acc(const float16v& a, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)a[8 * s + j];
  return r;
}
// row (of the 32-row accumulator tile) held by register i of lane half h
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
// value of x in lane l ^ 32 (one permlane32 swap + select)
__device__ __forceinline__ float xor32(float x) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float((threadIdx.x & 32) ? s[0] : s[1]);
}

// two ds_read_b64_tr_b16 halves (byte offsets lo / hi from base) as one MFMA operand; each caller's swizzle decides
// the offsets
__device__ __forceinline__ bf16x8 tr16_pair(const char* base, int lo_off, int hi_off) {
  const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(base + lo_off));
  const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(base + hi_off));
  short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
