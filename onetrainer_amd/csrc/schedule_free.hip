// Fused schedule-free AdamW (Defazio et al., "The Road Less Scheduled") over a flat parameter store: the step the
// reference asks of schedulefree.AdamWScheduleFree at modules/util/create.py:752-767 (its non-foreach path), and the
// two mode switches optimizer.eval() / optimizer.train() the reference trainer calls around every backup and save.
// The schedulefree package is not part of the reference tree, so the contract is that step as restated, in float64
// with the fp32 roundings named, by tests/_oracle_schedule_free.py; nothing here was compared with the package.
//
// The store holds the gradient point y while training; z (the base iterate) and v (exp_avg_sq) are fp32 states
// indexed as the store.  The averaged weights x are never stored: x = y + (1 - 1/beta1) (z - y).
//   sf_step   one launch over the store.  Per group the host passes lr (after the warm-up), ckp1 = weight / weight_sum,
//             a_y = lr (beta1 (1 - ckp1) - 1), beta2, 1 - beta2, 1 / bc2, eps and weight_decay; per element, with g
//             the gradient after the pending clip:
//               v  = beta2 v + (1 - beta2) g g
//               gn = g / (sqrt(v (1 / bc2)) + eps) + weight_decay y            (y before the update)
//               y  = y + ckp1 (z - y);   y = y + a_y gn;   z = z - lr gn
//             On a group's first step z = y is taken from the parameters instead of read.
//   sf_swap   p = p + w (z - p) over group ranges: w = 1 - 1/beta1 turns y into x, w = 1 - beta1 turns x into y.
// Both write the parameters through fs_write_params (flat_store.h): fp32; fp32 master + its RNE bf16 working copy;
// bf16 RNE or stochastic (the swap always RNE: a mode switch must be repeatable).
//
// Numerics: every fp32 operation above is one rounding in the order written (t = a * b; r = t + c: no fused
// multiply-add, compile with -ffp-contract=off), sqrtf and the division are the correctly rounded ones.
//
// HBM traffic per element: read y, g, z, v and write y, z, v -- AdamW's bytes on the fp32 and master forms (16 + 12 B,
// master 14 + 14 B); a bf16 store keeps z and v in fp32 (12 + 10 B against AdamW's 8 + 6 B).  The first step does not
// read z.  No atomics, no reductions.
#include "flat_store.h"

#define SF_THREADS 256

struct SfGroup {
  long long begin, end;   // element range [begin, end) of this group in the flat store; begin a multiple of 8
  float lr;               // group lr after the warm-up factor
  float a_y;              // lr (beta1 (1 - ckp1) - 1)
  float ckp1;             // weight / weight_sum
  float beta2;
  float one_minus_beta2;
  float inv_bc2;          // 1 / (1 - beta2^(k+1))
  float eps;
  float weight_decay;
  int first;              // the first step: z = y instead of a read (one value for every group of a launch)
  int pad;
};
struct SfGroups {
  SfGroup g[FS_MAX_GROUPS];
  int n;
};
struct SfSwapGroup {
  long long begin, end;
  float w;
  int pad;
};
struct SfSwapGroups {
  SfSwapGroup g[FS_MAX_GROUPS];
  int n;
};

// FORM 0: bf16 store (RNE or stochastic); 1: fp32 store; 2: fp32 master P + bf16 working copy W = rne(master).
// [v0, v1): the 8-element vectors of the launch window, global indices.  FIRST: the first step (every group's flag;
// the host passes one value for the whole store): z = y is taken from the parameters instead of read.  The loads do
// not wait for the group look-up: every vector of the window lies inside the store.
template <typename TP, typename TG, int FORM, bool FIRST>
__global__ void __launch_bounds__(SF_THREADS)
    sf_step_kernel(TP* __restrict__ P, bf16_t* __restrict__ W, const TG* __restrict__ Gr, float* __restrict__ Z,
                   float* __restrict__ V, long long v0, long long v1, SfGroups groups,
                   const float* __restrict__ clip_coef, int sr, unsigned long long seed) {
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const uint32_t key = fs_seed_key(seed);
  const long long stride = (long long)gridDim.x * SF_THREADS;
  for (long long i = v0 + blockIdx.x * (long long)SF_THREADS + threadIdx.x; i < v1; i += stride) {
    const long long e0 = i * 8;
    float y[8], g[8], z[8], v[8];
    fs_load8<TP>(P, e0, y);
    fs_load8<TG>(Gr, e0, g);
    fs_load8<float>(V, e0, v);
    if constexpr (!FIRST) fs_load8<float>(Z, e0, z);
    const SfGroup& G = groups.g[fs_find_group(groups, e0)];
    const unsigned valid = fs_valid(e0, G.begin, G.end);
    if (valid == 0u) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gg = fs_clip<FORM == 0>(g[j], coef, clip);
      const float zz = FIRST ? y[j] : z[j];
      const float t1 = G.beta2 * v[j], t2 = (G.one_minus_beta2 * gg) * gg;
      v[j] = t1 + t2;
      const float den = sqrtf(v[j] * G.inv_bc2) + G.eps;
      const float q = gg / den, wy = G.weight_decay * y[j];
      const float gn = q + wy;
      const float dz = zz - y[j];
      const float t3 = G.ckp1 * dz;
      float yy = y[j] + t3;
      const float t4 = G.a_y * gn;
      yy = yy + t4;
      const float t5 = G.lr * gn;
      z[j] = zz - t5;
      y[j] = yy;
    }
    fs_store8(V, e0, v, valid);
    fs_store8(Z, e0, z, valid);
    fs_write_params<FORM>(P, W, e0, y, valid, sr, key);
  }
}

template <typename TP, int FORM>
__global__ void __launch_bounds__(SF_THREADS)
    sf_swap_kernel(TP* __restrict__ P, bf16_t* __restrict__ W, const float* __restrict__ Z, long long v0, long long v1,
                   SfSwapGroups groups) {
  const long long stride = (long long)gridDim.x * SF_THREADS;
  for (long long i = v0 + blockIdx.x * (long long)SF_THREADS + threadIdx.x; i < v1; i += stride) {
    const long long e0 = i * 8;
    float p[8], z[8];
    fs_load8<TP>(P, e0, p);
    fs_load8<float>(Z, e0, z);
    const SfSwapGroup& G = groups.g[fs_find_group(groups, e0)];
    const unsigned valid = fs_valid(e0, G.begin, G.end);
    if (valid == 0u) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = z[j] - p[j];
      const float t = G.w * d;
      p[j] = p[j] + t;
    }
    fs_write_params<FORM>(P, W, e0, p, valid, 0, 0u);
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_sf_group_size(void) { return (int)sizeof(SfGroup); }
OTAMD_API int otamd_sf_swap_group_size(void) { return (int)sizeof(SfSwapGroup); }

// workgroups of a launch over nvec vectors, under the cap adamw.hip honours (fs_grid, flat_store.h)
static int sf_blocks(long long nvec) { return fs_grid(nvec, SF_THREADS, 256 * 16); }

// form 0: p, g bf16; 1: p, g fp32; 2: p the fp32 master, g bf16, w16 its bf16 working copy.  z / v: fp32, indexed as
// the store.  n: elements of the store (a multiple of 8); [begin, end): the window of this launch, multiples of 8.
OTAMD_API int otamd_sf_adamw_step(void* p, void* w16, const void* g, int form, float* z, float* v, long long n,
                                  long long begin, long long end, const SfGroup* groups, int n_groups,
                                  const float* clip_coef, int stochastic_rounding, unsigned long long seed,
                                  hipStream_t stream) {
  if (!p || !g || !z || !v || !fs_form_ok(form, w16) || !fs_window_ok(n, begin, end) ||
      !fs_groups_ok(groups, n_groups, n))
    return OTAMD_EINVAL;
  if (!fs_aligned16(p, w16, g, z, v)) return OTAMD_EINVAL;
  if (end == begin) return OTAMD_OK;
  const SfGroups G = fs_groups_arg<SfGroups>(groups, n_groups);
  for (int i = 1; i < n_groups; ++i)
    if ((groups[i].first != 0) != (groups[0].first != 0)) return OTAMD_EINVAL;   // one first step for the whole store
  const long long v0 = begin / 8, v1 = end / 8;
  const int blocks = sf_blocks(v1 - v0);
  const bool first = groups[0].first != 0;
  fs_dispatch(form, [&](auto F) {
    using TP = typename decltype(F)::TP;
    using TG = typename decltype(F)::TG;
    auto* kernel = first ? sf_step_kernel<TP, TG, F.form, true> : sf_step_kernel<TP, TG, F.form, false>;
    kernel<<<blocks, SF_THREADS, 0, stream>>>((TP*)p, F.w(w16), (const TG*)g, z, v, v0, v1, G, clip_coef,
                                              F.sr(stochastic_rounding), seed);
  });
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

OTAMD_API int otamd_sf_swap(void* p, void* w16, int form, const float* z, long long n, long long begin, long long end,
                            const SfSwapGroup* groups, int n_groups, hipStream_t stream) {
  if (!p || !z || !fs_form_ok(form, w16) || !fs_window_ok(n, begin, end) || !fs_groups_ok(groups, n_groups, n))
    return OTAMD_EINVAL;
  if (!fs_aligned16(p, w16, z)) return OTAMD_EINVAL;
  if (end == begin) return OTAMD_OK;
  const SfSwapGroups G = fs_groups_arg<SfSwapGroups>(groups, n_groups);
  const long long v0 = begin / 8, v1 = end / 8;
  const int blocks = sf_blocks(v1 - v0);
  fs_dispatch(form, [&](auto F) {
    using TP = typename decltype(F)::TP;
    sf_swap_kernel<TP, F.form><<<blocks, SF_THREADS, 0, stream>>>((TP*)p, F.w(w16), z, v0, v1, G);
  });
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
