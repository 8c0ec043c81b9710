// Fused 8-bit AdamW over a flat parameter store: the step the reference asks of bnb.optim.AdamW8bit at
// modules/util/create.py:553-566.  bitsandbytes is not part of the reference tree, so the contract is the published
// algorithm (Dettmers et al., "8-bit Optimizers via Block-wise Quantization": two states, blocks of 256, dynamic-tree
// codebooks) as restated by tests/_oracle_adamw8bit.py; nothing here was compared with the package.
//
// Layout.  A segment is one tensor of the store (A8Seg, a host-built table sorted by `begin`).  Its elements are cut
// into work blocks of 256 that start at the tensor's first element, numbered consecutively through the table (blk0),
// so a block never straddles two tensors or two parameter groups.  A tensor of at least min_8bit_size elements keeps
//   code1 / code2   one uint8 per element, indexed as the store (the store's padding is never written: it keeps the
//                   code the host filled in, the code of 0)
//   absmax1 / 2     one fp32 per block at state_off + (block - blk0)
// a smaller tensor keeps fp32 moments in the side buffers m32 / v32 at state_off + (element - begin).
//
// One wave64 owns one block: 4 elements per lane (16-byte loads on fp32, one 4-byte load of each code array), both
// maxima reduced across the wave with lane shuffles, no __syncthreads in the block loop.  Four blocks per workgroup,
// grid-stride.  The two codebooks and their midpoints sit in LDS (4 KB): decoding is one LDS read, encoding an 8-step
// binary search over the midpoints after one division by the block's maximum.
//
// Per element, g after the pending clip, scalars of the tensor's group rounded to fp32 by the host:
//   m = map1[code1] * absmax1;  v = map2[code2] * absmax2              (8-bit; fp32 tensors read m, v)
//   m = beta1 m + (1 - beta1) g;   v = beta2 v + ((1 - beta2) g) g
//   p = (p + step_size (m / (sqrt(v) + eps_c))) wd_factor
//       step_size = -lr sqrt(bc2) / bc1,  eps_c = sqrt(bc2) eps,  wd_factor = 1 - lr weight_decay
//   absmax1' = max |m|, absmax2' = max v over the block's elements
//   code1' = #{i : mid1[i] < m / absmax1'},  mid1[i] = (map1[i] + map1[i + 1]) 0.5   (0 / 0 taken as 0); code2' alike
// so a value on a midpoint takes the lower code.  Every fp32 operation is one rounding in the order written (no fused
// multiply-add: compile with -ffp-contract=off); sqrtf and the divisions are the correctly rounded ones.
//
// HBM traffic per element, fp32 store: read p, g (8 B) and two codes, write p (4 B) and two codes: 16 B plus 16 B
// of absmax per 256 elements, against 28 B of the fp32-state step in adamw.hip.
#include "flat_store.h"

#define A8_THREADS 256
#define A8_BLOCK 256

struct A8Seg {
  long long begin, end;   // element range [begin, end) of the tensor in the flat store; begin a multiple of 8
  long long blk0;         // its first work block; the next segment's is blk0 + ceil((end - begin) / 256)
  long long state_off;    // 8-bit: first entry in absmax1 / absmax2; fp32: first element in m32 / v32 (multiple of 8)
  int is8bit;
  int group;
};
struct A8Group {
  float beta1, one_minus_beta1, beta2, one_minus_beta2;
  float eps_c;       // sqrt(bc2) eps
  float step_size;   // -lr sqrt(bc2) / bc1
  float wd_factor;   // 1 - lr weight_decay
  float pad;
};
struct A8Groups {
  A8Group g[FS_MAX_GROUPS];
  int n;
};

template <typename T> __device__ __forceinline__ void a8_load4(const T* base, long long e, float* f);
template <> __device__ __forceinline__ void a8_load4<float>(const float* base, long long e, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(base + e);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
}
template <> __device__ __forceinline__ void a8_load4<bf16_t>(const bf16_t* base, long long e, float* f) {
  const uint2 a = *reinterpret_cast<const uint2*>(base + e);
  f[0] = __uint_as_float(a.x << 16); f[1] = __uint_as_float(a.x & 0xffff0000u);
  f[2] = __uint_as_float(a.y << 16); f[3] = __uint_as_float(a.y & 0xffff0000u);
}
// nv: how many of the four belong to the tensor; a partial vector is written element-wise (the next tensor's bytes
// and the padding stay untouched)
__device__ __forceinline__ void a8_store4(float* base, long long e, const float* x, int nv) {
  if (nv == 4) {
    *reinterpret_cast<float4*>(base + e) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
    for (int j = 0; j < nv; ++j) base[e + j] = x[j];
  }
}
__device__ __forceinline__ void a8_store4(bf16_t* base, long long e, const float* x, int nv) {
  if (nv == 4) {
    uint2 a;
    a.x = (uint32_t)f2bf(x[0]) | ((uint32_t)f2bf(x[1]) << 16);
    a.y = (uint32_t)f2bf(x[2]) | ((uint32_t)f2bf(x[3]) << 16);
    *reinterpret_cast<uint2*>(base + e) = a;
  } else {
    for (int j = 0; j < nv; ++j) base[e + j] = f2bf(x[j]);
  }
}
__device__ __forceinline__ void a8_store_codes(uint8_t* base, long long e, const uint32_t* c, int nv) {
  if (nv == 4) {
    *reinterpret_cast<uint32_t*>(base + e) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  } else {
    for (int j = 0; j < nv; ++j) base[e + j] = (uint8_t)c[j];
  }
}

// the code of q: how many of the 255 midpoints lie strictly below it
__device__ __forceinline__ uint32_t a8_encode(const float* mid, float q) {
  uint32_t c = 0;
#pragma unroll
  for (uint32_t bit = 128; bit > 0; bit >>= 1)
    if (mid[c + bit - 1] < q) c += bit;
  return c;
}

// FORM 0: bf16 store (RNE or stochastic); 1: fp32 store; 2: fp32 master P + bf16 working copy W = rne(master).
template <typename TP, typename TG, int FORM>
__global__ void __launch_bounds__(A8_THREADS)
    a8_step_kernel(TP* __restrict__ P, bf16_t* __restrict__ W, const TG* __restrict__ Gr, uint8_t* __restrict__ C1,
                   uint8_t* __restrict__ C2, float* __restrict__ A1, float* __restrict__ A2, float* __restrict__ M32,
                   float* __restrict__ V32, const float* __restrict__ qmap, const A8Seg* __restrict__ segs, int n_segs,
                   long long n_blocks, A8Groups groups, const float* __restrict__ clip_coef, int sr,
                   unsigned long long seed) {
  __shared__ float s_map1[256], s_map2[256], s_mid1[256], s_mid2[256];
  {
    const int t = threadIdx.x;
    s_map1[t] = qmap[t];
    s_map2[t] = qmap[256 + t];
    s_mid1[t] = t < 255 ? (qmap[t] + qmap[t + 1]) * 0.5f : __builtin_inff();
    s_mid2[t] = t < 255 ? (qmap[256 + t] + qmap[256 + t + 1]) * 0.5f : __builtin_inff();
  }
  __syncthreads();
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const uint32_t key = fs_seed_key(seed);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * (A8_THREADS / 64);
  for (long long b = (long long)blockIdx.x * (A8_THREADS / 64) + wave; b < n_blocks; b += stride) {
    // the last segment whose first block is not behind b (the host checked that the numbering is consecutive)
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const A8Seg S = segs[lo];
    const A8Group& G = groups.g[S.group];
    const long long lb = b - S.blk0;
    const long long e0 = S.begin + lb * A8_BLOCK + lane * 4;
    const long long left = S.end - e0;
    const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    float p[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    const long long s0 = S.state_off + (S.is8bit ? lb : lb * A8_BLOCK + lane * 4);
    if (nv > 0) {   // a vector that begins inside the tensor ends inside the store (tensors and the store pad to 8)
      a8_load4<TP>(P, e0, p);
      a8_load4<TG>(Gr, e0, g);
      if (S.is8bit) {
        const uint32_t c1 = *reinterpret_cast<const uint32_t*>(C1 + e0);
        const uint32_t c2 = *reinterpret_cast<const uint32_t*>(C2 + e0);
        const float a1 = A1[s0], a2 = A2[s0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          m[j] = s_map1[(c1 >> (8 * j)) & 255u] * a1;
          v[j] = s_map2[(c2 >> (8 * j)) & 255u] * a2;
        }
      } else {
        a8_load4<float>(M32, s0, m);
        a8_load4<float>(V32, s0, v);
      }
    }
    float mx1 = 0.f, mx2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = clip ? (FORM == 0 ? rbf(g[j] * coef) : g[j] * coef) : g[j];
      const float t1 = G.beta1 * m[j], t2 = G.one_minus_beta1 * gg;
      m[j] = t1 + t2;
      const float t3 = G.beta2 * v[j], t4 = (G.one_minus_beta2 * gg) * gg;
      v[j] = t3 + t4;
      const float den = sqrtf(v[j]) + G.eps_c;
      const float q = m[j] / den;
      const float t5 = G.step_size * q;
      const float pp = p[j] + t5;
      p[j] = pp * G.wd_factor;
      if (j < nv) {
        mx1 = fmaxf(mx1, fabsf(m[j]));
        mx2 = fmaxf(mx2, v[j]);
      }
    }
    if (S.is8bit) {
      mx1 = wave_max(mx1);
      mx2 = wave_max(mx2);
      if (nv > 0) {
        uint32_t c1[4], c2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float q1 = mx1 > 0.f ? m[j] / mx1 : 0.f;
          const float q2 = mx2 > 0.f ? v[j] / mx2 : 0.f;
          c1[j] = a8_encode(s_mid1, q1);
          c2[j] = a8_encode(s_mid2, q2);
        }
        a8_store_codes(C1, e0, c1, nv);
        a8_store_codes(C2, e0, c2, nv);
        if (lane == 0) {
          A1[s0] = mx1;
          A2[s0] = mx2;
        }
      }
    } else if (nv > 0) {
      a8_store4(M32, s0, m, nv);
      a8_store4(V32, s0, v, nv);
    }
    if (nv > 0) {
      if constexpr (FORM == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          p[j] = sr ? __uint_as_float((__float_as_uint(p[j]) + sr_bits(key, (uint64_t)(e0 + j))) & 0xFFFF0000u)
                    : rbf(p[j]);
      }
      a8_store4(P, e0, p, nv);
      if constexpr (FORM == 2) a8_store4(W, e0, p, nv);
    }
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_adamw8bit_seg_size(void) { return (int)sizeof(A8Seg); }
OTAMD_API int otamd_adamw8bit_group_size(void) { return (int)sizeof(A8Group); }

// The kernel trusts the table: every range it names lies inside its buffer, tensors are sorted and disjoint, the work
// blocks are numbered consecutively from 0, and state ranges of one kind do not overlap.  n: elements of the store;
// n_absmax: entries of absmax1 / absmax2; n_f32: elements of m32 / v32.  Host code only: launches nothing.
OTAMD_API int otamd_adamw8bit_check(const A8Seg* t, int n_segs, long long n, long long n_absmax, long long n_f32,
                                    int n_groups) {
  if (!t || n_segs < 1 || n < 0 || (n % 8) != 0 || n_absmax < 0 || n_f32 < 0 || !fs_group_count_ok(n_groups))
    return OTAMD_EINVAL;
  long long prev_end = 0, next_blk = 0, next_abs = 0, next_f32 = 0;
  for (int i = 0; i < n_segs; ++i) {
    const A8Seg& s = t[i];
    if (s.begin < prev_end || s.end <= s.begin || s.end > n || (s.begin % 8) != 0) return OTAMD_EINVAL;
    if (s.group < 0 || s.group >= n_groups) return OTAMD_EINVAL;
    if (s.blk0 != next_blk) return OTAMD_EINVAL;
    const long long numel = s.end - s.begin, nblk = (numel + A8_BLOCK - 1) / A8_BLOCK;
    if (s.is8bit) {
      if (s.state_off < next_abs || s.state_off + nblk > n_absmax) return OTAMD_EINVAL;
      next_abs = s.state_off + nblk;
    } else {
      const long long padded = (numel + 7) / 8 * 8;   // 4-wide loads that begin inside the tensor end inside this
      if (s.state_off < next_f32 || (s.state_off % 8) != 0 || s.state_off + padded > n_f32) return OTAMD_EINVAL;
      next_f32 = s.state_off + padded;
    }
    prev_end = s.end;
    next_blk += nblk;
  }
  return OTAMD_OK;
}

// form 0: p, g bf16; 1: p, g fp32; 2: p the fp32 master, g bf16, w16 its bf16 working copy.  code1 / code2: uint8,
// n elements; absmax1 / absmax2: fp32, n_absmax; m32 / v32: fp32, n_f32 (may be null when n_f32 == 0); qmap: 512 fp32
// on the device, the signed codebook then the unsigned one, each ascending.  table_dev / table_host: the same
// A8Seg[n_segs] on the device and on the host (checked here on every call).
OTAMD_API int otamd_adamw8bit_step(void* p, void* w16, const void* g, int form, void* code1, void* code2,
                                   float* absmax1, float* absmax2, long long n_absmax, float* m32, float* v32,
                                   long long n_f32, const float* qmap, long long n, const void* table_dev,
                                   const void* table_host, int n_segs, const A8Group* groups, int n_groups,
                                   const float* clip_coef, int stochastic_rounding, unsigned long long seed,
                                   hipStream_t stream) {
  if (!p || !g || !code1 || !code2 || !qmap || !table_dev || !table_host || !groups || !fs_form_ok(form, w16))
    return OTAMD_EINVAL;
  if ((n_absmax > 0 && (!absmax1 || !absmax2)) || (n_f32 > 0 && (!m32 || !v32))) return OTAMD_EINVAL;
  if (!fs_aligned16(p, w16, g, code1, code2, m32, v32)) return OTAMD_EINVAL;
  const A8Seg* t = (const A8Seg*)table_host;
  if (const int rc = otamd_adamw8bit_check(t, n_segs, n, n_absmax, n_f32, n_groups)) return rc;
  const A8Seg& l = t[n_segs - 1];
  const long long n_blocks = l.blk0 + (l.end - l.begin + A8_BLOCK - 1) / A8_BLOCK;
  const A8Groups G = fs_groups_arg<A8Groups>(groups, n_groups);
  const int blocks = fs_grid(n_blocks, A8_THREADS / 64, 256 * 16);   // a wave per block; the cap adamw.hip honours
  fs_dispatch(form, [&](auto F) {
    using TP = typename decltype(F)::TP;
    using TG = typename decltype(F)::TG;
    a8_step_kernel<TP, TG, F.form><<<blocks, A8_THREADS, 0, stream>>>(
        (TP*)p, F.w(w16), (const TG*)g, (uint8_t*)code1, (uint8_t*)code2, absmax1, absmax2, m32, v32, qmap,
        (const A8Seg*)table_dev, n_segs, n_blocks, G, clip_coef, F.sr(stochastic_rounding), seed);
  });
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
