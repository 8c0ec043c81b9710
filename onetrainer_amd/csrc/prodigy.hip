// Fused Prodigy (Mishchenko and Defazio, "Prodigy: an expeditiously adaptive parameter-free learner") over a flat
// parameter store: the step the reference asks of prodigyopt.Prodigy at modules/util/create.py:863-881.  That package
// is not part of the reference tree, so the contract is the published step as restated, in float64 with the fp32
// roundings named, by tests/_oracle_prodigy.py; nothing here was compared with the package itself.
//
// Prodigy's step size d is a ratio of two sums over the whole store, and the parameter update needs the new d, so a
// step is three launches with the scalars handed over on the device (ProdigyState); the host reads nothing back:
//   prodigy_accumulate  one workgroup per NormChunk (the grad-norm chunk table: <= 65536 elements, 8-aligned begin,
//                       never across a tensor).  Per element, with g the gradient after the pending clip and the old d:
//                         num += g (p0 - p)        p0 - p in fp32, the product and the sum in fp64
//                         m = beta1 m + d (1 - beta1) g           (beta1 > 0)
//                         v = beta2 v + d^2 (1 - beta2) g g
//                         s = beta3 s + a g,   a = (d / d0) dlr, or (d / d0) d under safeguard_warmup
//                         den += |s|
//                       into chunk_num[c], chunk_den[c]: one fp64 slot per chunk, no atomics, the same bits every run.
//   prodigy_finalize    one workgroup folds the slots in a fixed order and does the scalar part in fp64:
//                         d_numerator = beta3 d_numerator + (d / d0) dlr num;  d_denom = den
//                         den == 0: skip = 1, nothing else changes (no update, k stays)
//                         d_hat = d_coef d_numerator / d_denom;  d == d0: d = max(d, d_hat);  d_max = max(d_max, d_hat)
//                         d = min(d_max, d growth_rate);  k += 1
//                       and leaves d, dlr (from the OLD d) and skip for the next launch.
//   prodigy_apply       grid-stride over the store (workgroup cap OTAMD_ADAMW_BLOCKS, as adamw.hip):
//                         p = p + (-weight_decay dlr) p                    (decoupled decay)
//                         p = p - dlr m / (sqrt(v) + d eps)                new d, old dlr; beta1 == 0: d g for m
//                       written through fs_write_params (flat_store.h: fp32; fp32 master + RNE bf16 working copy; bf16 RNE or stochastic).
//
// Numerics: m, v, s and p0 are fp32 for every store form; every fp32 operation above is one rounding, in the order
// written (t = a * b; r = t + c: no fused multiply-add), so compile with -ffp-contract=off.  The per-element
// coefficients are formed in fp64 from the device scalars and rounded to fp32 once.
//
// HBM traffic per fp32 element: accumulate reads p, g, p0, m, v, s (24 B) and writes m, v, s (12 B); apply reads
// p, m, v (12 B) and writes p (4 B).  A master store reads g as bf16 (-2 B) and also writes the bf16 working copy
// (+2 B); a bf16 store reads and writes p and g as bf16.  The first step writes p0 instead of reading it.
#include "flat_store.h"

#include <cmath>

#define PRODIGY_THREADS 256

struct ProdigyState {   // device resident; the host writes it at start-up and on load_state_dict only
  double d, d_max, d_numerator, d_denom, d_hat;
  double dlr;    // d lr bc of the step in flight, from d before that step
  double k;      // completed steps (exact in a double)
  double skip;   // 1: the step in flight found d_denom == 0 and updates nothing
};
struct ProdigyHyper {
  double lr, beta1, beta2, beta3, eps, weight_decay, d0, d_coef, growth_rate;
  int decouple, use_bias_correction, safeguard_warmup, pad;
};

// dlr = d lr bc, bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) under use_bias_correction: a function of the state
// and the launch arguments alone, so accumulate and finalize form the same bits
__device__ __forceinline__ double prodigy_dlr(double d, double k, const ProdigyHyper& H) {
  double bc = 1.0;
  if (H.use_bias_correction) bc = sqrt(1.0 - pow(H.beta2, k + 1.0)) / (1.0 - pow(H.beta1, k + 1.0));
  return d * H.lr * bc;
}

// g after the pending clip and, for the coupled form of weight decay, g + weight_decay p
template <bool BFROUND>
__device__ __forceinline__ float prodigy_grad(float g, float p, float coef, bool clip, float wd_coupled) {
  g = fs_clip<BFROUND>(g, coef, clip);
  if (wd_coupled != 0.f) {
    const float t = wd_coupled * p;
    g = g + t;
  }
  return g;
}

// ---- 1: states and the two sums -----------------------------------------------------------------------------------
// capture: the first step: p0 = p is written instead of read (p0 - p = 0)
template <typename TP, typename TG, bool BFROUND>
__global__ void __launch_bounds__(PRODIGY_THREADS)
    prodigy_accumulate_kernel(const TP* __restrict__ P, const TG* __restrict__ Gr, float* __restrict__ P0,
                              float* __restrict__ M, float* __restrict__ V, float* __restrict__ Sx,
                              const NormChunk* __restrict__ chunks, double* __restrict__ chunk_num,
                              double* __restrict__ chunk_den, const ProdigyState* __restrict__ S, ProdigyHyper H,
                              const float* __restrict__ clip_coef, int capture) {
  __shared__ double red[8];
  const NormChunk c = chunks[blockIdx.x];
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const double d = S->d;
  const double dlr = prodigy_dlr(d, S->k, H);
  const double r = d / H.d0;
  const bool has_m = H.beta1 > 0.0;
  const float b1 = (float)H.beta1, b2 = (float)H.beta2, b3 = (float)H.beta3;
  const float c_m = (float)(d * (1.0 - H.beta1));
  const float c_v = (float)(d * d * (1.0 - H.beta2));
  const float a = (float)(H.safeguard_warmup ? r * d : r * dlr);
  const float wdc = (!H.decouple && H.weight_decay != 0.0) ? (float)H.weight_decay : 0.f;
  double num = 0.0, den = 0.0;
  for (long long e = c.begin + 8 * threadIdx.x; e < c.end; e += 8 * PRODIGY_THREADS) {
    float p[8], g[8], p0[8], m[8], v[8], s[8];
    fs_load8<TP>(P, e, p);
    fs_load8<TG>(Gr, e, g);
    if (!capture) fs_load8<float>(P0, e, p0);
    if (has_m) fs_load8<float>(M, e, m);
    fs_load8<float>(V, e, v);
    fs_load8<float>(Sx, e, s);
    const unsigned valid = e + 8 <= c.end ? 0xFFu : (1u << (int)(c.end - e)) - 1u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = valid >> j & 1;
      const float gg = prodigy_grad<BFROUND>(g[j], p[j], coef, clip, wdc);
      if (capture) {
        p0[j] = p[j];
      } else {
        const float diff = p0[j] - p[j];
        const double t = (double)gg * (double)diff;
        num += ok ? t : 0.0;
      }
      if (has_m) {
        const float t1 = b1 * m[j], t2 = c_m * gg;
        m[j] = t1 + t2;
      }
      const float t3 = b2 * v[j], t4 = (c_v * gg) * gg;
      v[j] = t3 + t4;
      const float t5 = b3 * s[j], t6 = a * gg;
      s[j] = t5 + t6;
      den += ok ? (double)fabsf(s[j]) : 0.0;
    }
    if (capture) fs_store8(P0, e, p0, valid);
    if (has_m) fs_store8(M, e, m, valid);
    fs_store8(V, e, v, valid);
    fs_store8(Sx, e, s, valid);
  }
  num = wave_sum_d(num);
  den = wave_sum_d(den);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = num;
    red[4 + (threadIdx.x >> 6)] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    chunk_num[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    chunk_den[blockIdx.x] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// ---- 2: the scalars -------------------------------------------------------------------------------------------------
// thread t adds slots t, t + 256, ... in index order, then the wave and LDS folds of accumulate: a fixed tree
__global__ void __launch_bounds__(PRODIGY_THREADS)
    prodigy_finalize_kernel(const double* __restrict__ chunk_num, const double* __restrict__ chunk_den, int n_chunks,
                            ProdigyState* __restrict__ S, ProdigyHyper H) {
  __shared__ double red[8];
  double num = 0.0, den = 0.0;
  for (int c = threadIdx.x; c < n_chunks; c += PRODIGY_THREADS) {
    num += chunk_num[c];
    den += chunk_den[c];
  }
  num = wave_sum_d(num);
  den = wave_sum_d(den);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = num;
    red[4 + (threadIdx.x >> 6)] = den;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  num = (red[0] + red[1]) + (red[2] + red[3]);
  den = (red[4] + red[5]) + (red[6] + red[7]);
  double d = S->d;
  const double k = S->k;
  const double dlr = prodigy_dlr(d, k, H);
  const double d_numerator = H.beta3 * S->d_numerator + ((d / H.d0) * dlr) * num;
  S->d_numerator = d_numerator;
  S->d_denom = den;
  S->dlr = dlr;
  if (den == 0.0) {
    S->skip = 1.0;
    return;
  }
  const double d_hat = H.d_coef * d_numerator / den;
  if (d == H.d0) d = fmax(d, d_hat);
  const double d_max = fmax(S->d_max, d_hat);
  d = fmin(d_max, d * H.growth_rate);
  S->d = d;
  S->d_max = d_max;
  S->d_hat = d_hat;
  S->k = k + 1.0;
  S->skip = 0.0;
}

// ---- 3: the parameters ----------------------------------------------------------------------------------------------
// FORM 0: bf16 store (RNE or stochastic); 1: fp32 store; 2: fp32 master + bf16 working copy W = rne(master).
// n8: 8-element vectors of the store (the store pads every tensor to 8 elements; the padding holds zeros: p = m = 0
// and d eps > 0 leave them zeros)
template <typename TP, typename TG, int FORM>
__global__ void __launch_bounds__(PRODIGY_THREADS)
    prodigy_apply_kernel(TP* __restrict__ P, bf16_t* __restrict__ W, const float* __restrict__ M,
                         const float* __restrict__ V, const TG* __restrict__ Gr, long long n8,
                         const ProdigyState* __restrict__ S, ProdigyHyper H, const float* __restrict__ clip_coef, int sr,
                         unsigned long long seed) {
  if (S->skip != 0.0) return;
  const double d = S->d, dlr = S->dlr;
  const uint32_t k = fs_seed_key(seed);
  const bool has_m = H.beta1 > 0.0;
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const float df = (float)d, dlrf = (float)dlr, de = (float)(d * H.eps);
  const float wdd = (H.decouple && H.weight_decay != 0.0) ? (float)(-(H.weight_decay * dlr)) : 0.f;
  const float wdc = (!H.decouple && H.weight_decay != 0.0) ? (float)H.weight_decay : 0.f;
  const long long stride = (long long)gridDim.x * PRODIGY_THREADS;
  for (long long i = blockIdx.x * (long long)PRODIGY_THREADS + threadIdx.x; i < n8; i += stride) {
    const long long e = i * 8;
    float p[8], m[8], v[8];
    fs_load8<TP>(P, e, p);
    fs_load8<float>(V, e, v);
    if (has_m) {
      fs_load8<float>(M, e, m);
    } else {   // beta1 == 0: d g stands for the first moment (g as accumulate saw it: p is still the old one)
      float g[8];
      fs_load8<TG>(Gr, e, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = df * prodigy_grad<FORM == 0>(g[j], p[j], coef, clip, wdc);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float denom = sqrtf(v[j]) + de;
      float x = p[j];
      if (wdd != 0.f) {
        const float t = wdd * x;
        x = x + t;
      }
      const float u = (dlrf * m[j]) / denom;
      p[j] = x - u;
    }
    fs_write_params<FORM>(P, W, e, p, 0xFFu, sr, k);
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_prodigy_state_size(void) { return (int)sizeof(ProdigyState); }
OTAMD_API int otamd_prodigy_hyper_size(void) { return (int)sizeof(ProdigyHyper); }

static bool prodigy_hyper_ok(const ProdigyHyper* h) {
  return h && h->d0 > 0.0 && h->eps > 0.0 && h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0 &&
         h->beta3 >= 0.0 && h->beta3 <= 1.0;
}

// form 0: p, g bf16; 1: p, g fp32; 2: p the fp32 master, g bf16.  p0 / m / v / s: fp32, indexed as the store (m may be
// null when beta1 == 0).  chunks: device table of n_chunks NormChunk whose ranges the caller checked (8-aligned begin,
// inside the store, at most 65536 elements); chunk_num / chunk_den: double[n_chunks]; state: device ProdigyState.
OTAMD_API int otamd_prodigy_accumulate(const void* p, const void* g, int form, float* p0, float* m, float* v, float* s,
                                       const void* chunks, int n_chunks, double* chunk_num, double* chunk_den,
                                       const void* state, const ProdigyHyper* hyper, const float* clip_coef,
                                       int capture_p0, hipStream_t stream) {
  if (!p || !g || !p0 || !v || !s || !chunks || !chunk_num || !chunk_den || !state || form < 0 || form > 2 ||
      n_chunks < 0 || !prodigy_hyper_ok(hyper) || (hyper->beta1 > 0.0 && !m))
    return OTAMD_EINVAL;
  if (!fs_aligned16(p, g, p0, m, v, s)) return OTAMD_EINVAL;
  if (n_chunks == 0) return OTAMD_OK;
  fs_dispatch(form, [&](auto F) {
    using TP = typename decltype(F)::TP;
    using TG = typename decltype(F)::TG;
    prodigy_accumulate_kernel<TP, TG, F.form == 0><<<n_chunks, PRODIGY_THREADS, 0, stream>>>(
        (const TP*)p, (const TG*)g, p0, m, v, s, (const NormChunk*)chunks, chunk_num, chunk_den,
        (const ProdigyState*)state, *hyper, clip_coef, capture_p0);
  });
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

OTAMD_API int otamd_prodigy_finalize(const double* chunk_num, const double* chunk_den, int n_chunks, void* state,
                                     const ProdigyHyper* hyper, hipStream_t stream) {
  if (!state || n_chunks < 0 || (n_chunks > 0 && (!chunk_num || !chunk_den)) || !prodigy_hyper_ok(hyper))
    return OTAMD_EINVAL;
  prodigy_finalize_kernel<<<1, PRODIGY_THREADS, 0, stream>>>(chunk_num, chunk_den, n_chunks, (ProdigyState*)state,
                                                             *hyper);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// n: elements of the store (a multiple of 8).  w16: the bf16 working copy (form 2).  g and clip_coef are read when
// beta1 == 0 only (clip_coef: the coefficient accumulate applied, or null).
OTAMD_API int otamd_prodigy_apply(void* p, void* w16, const void* g, int form, const float* m, const float* v,
                                  long long n, const void* state, const ProdigyHyper* hyper, const float* clip_coef,
                                  int stochastic_rounding, unsigned long long seed, hipStream_t stream) {
  if (!p || !g || !v || !state || !fs_form_ok(form, w16) || n < 0 || (n % 8) != 0 || !prodigy_hyper_ok(hyper) ||
      (hyper->beta1 > 0.0 && !m))
    return OTAMD_EINVAL;
  if (!fs_aligned16(p, w16, g, m, v)) return OTAMD_EINVAL;
  if (n == 0) return OTAMD_OK;
  const long long n8 = n / 8;
  const int blocks = fs_grid(n8, PRODIGY_THREADS, 256 * 16);   // the cap adamw.hip honours
  fs_dispatch(form, [&](auto F) {
    using TP = typename decltype(F)::TP;
    using TG = typename decltype(F)::TG;
    prodigy_apply_kernel<TP, TG, F.form><<<blocks, PRODIGY_THREADS, 0, stream>>>(
        (TP*)p, F.w(w16), m, v, (const TG*)g, n8, (const ProdigyState*)state, *hyper, clip_coef,
        F.sr(stochastic_rounding), seed);
  });
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
