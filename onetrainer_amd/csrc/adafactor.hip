// Fused Adafactor (factored second moments) over a flat parameter store.  Replaces, per parameter tensor,
// the reference's
//   modules/util/optimizer/adafactor_extensions.py:16-95  (step_adafactor_parameter on transformers.Adafactor)
// built at modules/util/create.py:914-936, with FIVE launches over the whole store (the reference runs ~25 torch
// ops per tensor per step in a Python loop):
//   1 stats    row / column sums of g^2 + eps1 per slab, sum p^2 (scale_parameter); states that a slab owns
//              whole (unfactored tensors, matrices that fit one LDS stage) take their EMA update here
//   2 fold     matrices that span slabs: per-slab partials summed in slab order, EMA update, row-state means
//   3 unorm    sum u^2 per slab, u recomputed from g and the fresh states (never materialised)
//   4 scalars  per tensor: slab sums folded in slab order -> rms(p), rms(u)
//   5 apply    clip-threshold scaling, weight decay, parameter write (bf16 RNE or stochastic, fp32, fp32 master +
//              bf16 working copy)
// Every reduction has a fixed order (no atomics): two runs give the same bits.
//
// Layout.  A host-built tensor table (AdafactorTensor) and slab table (AdafactorSlab), built once.  A tensor of
// ndim >= 2 is `batch` matrices of rows x cols (its last two dimensions); one fp32 state buffer holds its row
// state (batch * rows), column state (batch * cols) or, for ndim < 2, a full state.  Slabs:
//   mode 0 (unfactored)  element ranges of the tensor
//   mode 1 (packed)      rows * cols <= AF_STAGE: a slab is whole matrices, AF_STAGE elements per LDS stage
//                        (3x3 conv kernels: 455 matrices a stage)
//   mode 2 (big)         rows [r0, r1) of one matrix x a column tile of <= AF_CT columns; row sums cross
//                        column tiles and column sums cross row slabs through the partial buffers
// Tensor offsets are 8-element aligned, rows are not: every global access is a 16-byte vector at an 8-aligned
// element index of the store, with the lanes outside the segment masked (partial vectors are written
// element-wise, so neighbouring slabs never write the same bytes).
//
// Arithmetic: fp32 element ops in the reference's order (-ffp-contract=off; the fused multiply-adds are the
// ones torch's CPU add_(alpha=) kernels use), fp32 sums.  tests/_oracle_adafactor.py restates it.
//
// The unorm kernel, the slab walk and the EMA are shared with came.hip and live in adafactor_walk.h; the masked loads
// and stores, the clip rounding and the parameter write are every flat-store optimizer's (flat_store.h).  The
// statistics kernel is not shared: came_stats_kernel (came.hip) restates its three-mode body.
#include "adafactor_walk.h"

struct AdafactorGroup {
  float lr;
  float neg_wd;              // -weight_decay
  float alpha_wd;            // -weight_decay * lr rounded once (scale_parameter off)
  float eps1, eps2, clip_threshold;
  float beta2t, one_minus_beta2t;   // 1 - step^decay_rate
  int scale_parameter;
  int pad;
};
struct AdafactorGroups { AdafactorGroup g[FS_MAX_GROUPS]; };

// ---- 1: statistics --------------------------------------------------------------------------------------------
template <typename TP, typename TG, bool BFROUND>
__global__ void __launch_bounds__(AF_THREADS) af_stats_kernel(const TP* __restrict__ P, const TG* __restrict__ Gr,
                                                              float* __restrict__ state, float* __restrict__ scratch,
                                                              double* __restrict__ slab_sq,
                                                              const AdafactorTensor* __restrict__ tensors,
                                                              const AdafactorSlab* __restrict__ slabs, int s0,
                                                              AdafactorGroups groups,
                                                              const float* __restrict__ clip_coef) {
  __shared__ __attribute__((aligned(16))) float s_stage[AF_STAGE + 16];
  __shared__ float s_acc[AF_STAGE];
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const int si = s0 + blockIdx.x;
  const AdafactorSlab sl = slabs[si];
  const AdafactorTensor T = tensors[sl.tensor];
  const AdafactorGroup G = groups.g[T.group];
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const bool scale = G.scale_parameter != 0;
  double pacc = 0.0;

  if (T.mode == 0) {
    for (long long i = sl.row0 + tid; i < sl.row1; i += AF_THREADS) {
      const float g = fs_clip<BFROUND>(fs_load1<TG>(Gr, T.offset + i), coef, clip);
      const float upd = g * g + G.eps1;
      float* v = state + T.full_off + i;
      *v = af_ema(*v, upd, G.beta2t, G.one_minus_beta2t);
      if (scale) {
        const float p = fs_load1<TP>(P, T.offset + i);
        pacc += (double)(p * p);
      }
    }
  } else if (T.mode == 1) {
    const int rc = T.rows * T.cols, mps = T.slab_rows;
    const long long m_begin = sl.row0 / T.rows, m_end = sl.row1 / T.rows;
    for (long long ms = m_begin; ms < m_end; ms += mps) {
      const int nm = (int)(m_end - ms < mps ? m_end - ms : mps);
      const long long e0 = T.offset + ms * rc, e1 = e0 + (long long)nm * rc;
      const long long a0 = e0 & ~7LL;
      const int sh = (int)(e0 - a0);
      __syncthreads();   // the previous stage's readers are done
      for (long long v = a0 + 8 * tid; v < e1; v += 8 * AF_THREADS) {
        float f[8];
        fs_load8<TG>(Gr, v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) s_stage[v - a0 + j] = fs_clip<BFROUND>(f[j], coef, clip);
        if (scale) {
          float q[8];
          fs_load8<TP>(P, v, q);
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (v + j >= e0 && v + j < e1) s = fmaf(q[j], q[j], s);
          pacc += (double)s;
        }
      }
      __syncthreads();
      const int nrows = nm * T.rows, ncols = nm * T.cols;
      for (int i = tid; i < nrows; i += AF_THREADS) {   // row i of the stage: elements [i * cols, (i + 1) * cols)
        const float* x = s_stage + sh + (long long)i * T.cols;
        float s = 0.f;
        for (int c = 0; c < T.cols; ++c) s += x[c] * x[c] + G.eps1;
        float* rs = state + T.row_off + ms * T.rows + i;
        const float nv = af_ema(*rs, s / (float)T.cols, G.beta2t, G.one_minus_beta2t);
        *rs = nv;
        s_acc[i] = nv;
      }
      for (int i = tid; i < ncols; i += AF_THREADS) {
        const int ml = i / T.cols, c = i - ml * T.cols;
        const float* x = s_stage + sh + ml * rc + c;
        float s = 0.f;
        for (int r = 0; r < T.rows; ++r) {
          const float g = x[r * T.cols];
          s += g * g + G.eps1;
        }
        float* cs = state + T.col_off + ms * T.cols + i;
        *cs = af_ema(*cs, s / (float)T.rows, G.beta2t, G.one_minus_beta2t);
      }
      __syncthreads();
      for (int m = tid; m < nm; m += AF_THREADS) {   // mean of the matrix's fresh row states
        float s = 0.f;
        for (int r = 0; r < T.rows; ++r) s += s_acc[m * T.rows + r];
        scratch[T.rmean_off + ms + m] = s / (float)T.rows;
      }
    }
  } else {
    const int width = sl.col1 - sl.col0;
    const int W8 = ((width + 7) / 8 + 1) * 8;   // padded row of the stage: the row's aligned vectors
    const int vpr = W8 / 8;
    const int stage_rows = AF_STAGE / W8 > 0 ? AF_STAGE / W8 : 1;
    const long long b = sl.row0 / T.rows;
    const int tile = sl.col0 / AF_CT;
    for (int c = tid; c < width; c += AF_THREADS) s_acc[c] = 0.f;
    for (long long r0 = sl.row0; r0 < sl.row1; r0 += stage_rows) {
      const int nr = (int)(sl.row1 - r0 < stage_rows ? sl.row1 - r0 : stage_rows);
      __syncthreads();
      for (int q = tid; q < nr * vpr; q += AF_THREADS) {
        const int i = q / vpr, j = q - i * vpr;
        const long long e0 = T.offset + (r0 + i) * T.cols + sl.col0, e1 = e0 + width;
        const long long v = (e0 & ~7LL) + 8 * j;
        if (v < e1) {
          float f[8];
          fs_load8<TG>(Gr, v, f);
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) s_stage[i * W8 + 8 * j + jj] = fs_clip<BFROUND>(f[jj], coef, clip);
          if (scale) {
            float p8[8];
            fs_load8<TP>(P, v, p8);
            float s = 0.f;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
              if (v + jj >= e0 && v + jj < e1) s = fmaf(p8[jj], p8[jj], s);
            pacc += (double)s;
          }
        }
      }
      __syncthreads();
      const int wave = tid >> 6, lane = tid & 63;
      for (int i = wave; i < nr; i += AF_THREADS / 64) {   // row sums over this tile's columns: a wave per row
        const int sh = (int)((T.offset + (r0 + i) * T.cols + sl.col0) & 7);
        const float* x = s_stage + i * W8 + sh;
        float s = 0.f;
        for (int c = lane; c < width; c += 64) s += x[c] * x[c] + G.eps1;
        s = wave_sum(s);
        if (lane == 0) scratch[T.rpart_off + (r0 + i) * T.col_tiles + tile] = s;
      }
      for (int c = tid; c < width; c += AF_THREADS) {      // column sums over the stage's rows: a thread per column
        float s = 0.f;
        for (int i = 0; i < nr; ++i) {
          const int sh = (int)((T.offset + (r0 + i) * T.cols + sl.col0) & 7);
          const float g = s_stage[i * W8 + sh + c];
          s += g * g + G.eps1;
        }
        s_acc[c] += s;   // each thread owns its columns
      }
    }
    const long long sidx = (sl.row0 - b * T.rows) / T.slab_rows;
    for (int c = tid; c < width; c += AF_THREADS)
      scratch[T.cpart_off + (b * T.row_slabs + sidx) * T.cols + sl.col0 + c] = s_acc[c];
  }
  if (scale) {
    const double t = af_block_sum_d(pacc, s_red);
    if (tid == 0) slab_sq[2 * (long long)si] = t;
  }
}

// ---- 2: fold the partials of the matrices that span slabs (one workgroup per tensor) ---------------------------
__global__ void __launch_bounds__(1024) af_fold_kernel(float* __restrict__ state, float* __restrict__ scratch,
                                                       const AdafactorTensor* __restrict__ tensors, int t0,
                                                       AdafactorGroups groups) {
  __shared__ float red[16];
  const AdafactorTensor T = tensors[t0 + blockIdx.x];
  if (T.mode != 2) return;
  const AdafactorGroup G = groups.g[T.group];
  const long long nrow = (long long)T.batch * T.rows, ncol = (long long)T.batch * T.cols;
  for (long long i = threadIdx.x; i < nrow; i += blockDim.x) {
    float s = 0.f;
    for (int j = 0; j < T.col_tiles; ++j) s += scratch[T.rpart_off + i * T.col_tiles + j];
    float* rs = state + T.row_off + i;
    *rs = af_ema(*rs, s / (float)T.cols, G.beta2t, G.one_minus_beta2t);
  }
  for (long long i = threadIdx.x; i < ncol; i += blockDim.x) {
    const long long b = i / T.cols;
    const int c = (int)(i - b * T.cols);
    float s = 0.f;
    for (int k = 0; k < T.row_slabs; ++k) s += scratch[T.cpart_off + (b * T.row_slabs + k) * T.cols + c];
    float* cs = state + T.col_off + i;
    *cs = af_ema(*cs, s / (float)T.rows, G.beta2t, G.one_minus_beta2t);
  }
  __threadfence_block();
  __syncthreads();
  for (int b = 0; b < T.batch; ++b) {
    float s = 0.f;
    for (int r = threadIdx.x; r < T.rows; r += blockDim.x) s += state[T.row_off + (long long)b * T.rows + r];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) scratch[T.rmean_off + b] = t / (float)T.rows;
    __syncthreads();
  }
}

// ---- 3: sum u^2 per slab: af_unorm_kernel<AdafactorGroup, ...> (adafactor_walk.h) -> slab_sq[2 s + 1] ----------

// ---- 4: per-tensor scalars: the slab sums in slab order -> scal[4 t] = rms(p), scal[4 t + 1] = rms(u) --------
__global__ void af_scalars_kernel(const double* __restrict__ slab_sq, float* __restrict__ scal,
                                  const AdafactorTensor* __restrict__ tensors, int t0, int t1, AdafactorGroups groups) {
  const int t = t0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= t1) return;
  const AdafactorTensor T = tensors[t];
  double sp = 0.0, su = 0.0;
  for (int s = T.slab0; s < T.slab0 + T.n_slabs; ++s) {
    sp += slab_sq[2 * (long long)s];
    su += slab_sq[2 * (long long)s + 1];
  }
  const float rn = (float)sqrt((double)T.numel);   // tensor.norm(2) / numel ** 0.5
  if (groups.g[T.group].scale_parameter) scal[4 * t] = (float)sqrt(sp) / rn;
  scal[4 * t + 1] = (float)sqrt(su) / rn;
}

// ---- 5: apply ---------------------------------------------------------------------------------------------------
// FORM 0: bf16 store (RNE or stochastic); 1: fp32 store; 2: fp32 master + bf16 working copy W = rne(master)
template <typename TP, typename TG, int FORM>
__global__ void __launch_bounds__(AF_THREADS) af_apply_kernel(TP* __restrict__ P, const TG* __restrict__ Gr,
                                                              bf16_t* __restrict__ W, const float* __restrict__ state,
                                                              const float* __restrict__ scratch,
                                                              const float* __restrict__ scal,
                                                              const AdafactorTensor* __restrict__ tensors,
                                                              const AdafactorSlab* __restrict__ slabs, int s0,
                                                              AdafactorGroups groups, const float* __restrict__ clip_coef,
                                                              int sr, unsigned long long seed) {
  __shared__ float s_r[AF_STAGE];
  __shared__ float s_c[AF_STAGE];
  const AdafactorSlab sl = slabs[s0 + blockIdx.x];
  const AdafactorTensor T = tensors[sl.tensor];
  const AdafactorGroup G = groups.g[T.group];
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const uint32_t k = fs_seed_key(seed);
  // update.div_((rms(update) / clip_threshold).clamp_(min=1.0)); lr = lr * max(eps2, RMS) (scale_parameter)
  const float denom = fmaxf(scal[4 * sl.tensor + 1] / G.clip_threshold, 1.f);
  const bool scale = G.scale_parameter != 0;
  const float lr = scale ? fmaxf(G.eps2, scal[4 * sl.tensor]) * G.lr : G.lr;
  const bool decay = G.neg_wd != 0.f;
  const float alpha = scale ? G.neg_wd * lr : G.alpha_wd;
  af_walk<TG, FORM == 0>(Gr, state, scratch, T, sl, coef, clip, s_r, s_c,
                         [&](long long v, const float* g, const float* fac, unsigned valid) {
                           float p[8];
                           fs_load8<TP>(P, v, p);
#pragma unroll
                           for (int j = 0; j < 8; ++j) {
                             float u = fac[j] * g[j];
                             u = u / denom;
                             u = u * lr;
                             float x = p[j];
                             if (decay) x = fmaf(x, alpha, x);   // p.add_(p, alpha=-weight_decay * lr)
                             p[j] = x - u;                       // p.add_(-update)
                           }
                           fs_write_params<FORM>(P, W, v, p, valid, sr, k);
                         });
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_adafactor_tensor_size(void) { return (int)sizeof(AdafactorTensor); }
OTAMD_API int otamd_adafactor_slab_size(void) { return (int)sizeof(AdafactorSlab); }
OTAMD_API int otamd_adafactor_group_size(void) { return (int)sizeof(AdafactorGroup); }

template <typename TP, typename TG, int FORM>
static int af_launch(void* p, const void* g, void* w, float* state, float* scratch, double* slab_sq, float* scal,
                     const AdafactorTensor* tensors, int t0, int t1, const AdafactorSlab* slabs, int s0, int s1,
                     const AdafactorGroups& G, const float* clip_coef, int sr, unsigned long long seed,
                     hipStream_t stream) {
  const int ns = s1 - s0, nt = t1 - t0;
  af_stats_kernel<TP, TG, FORM == 0><<<ns, AF_THREADS, 0, stream>>>((const TP*)p, (const TG*)g, state, scratch, slab_sq,
                                                                    tensors, slabs, s0, G, clip_coef);
  OTAMD_CHECK_LAUNCH();
  af_fold_kernel<<<nt, 1024, 0, stream>>>(state, scratch, tensors, t0, G);
  OTAMD_CHECK_LAUNCH();
  af_unorm_kernel<AdafactorGroup, TG, FORM == 0><<<ns, AF_THREADS, 0, stream>>>((const TG*)g, state, scratch, slab_sq, 2, 1,
                                                                                tensors, slabs, s0, clip_coef);
  OTAMD_CHECK_LAUNCH();
  af_scalars_kernel<<<(nt + 255) / 256, 256, 0, stream>>>(slab_sq, scal, tensors, t0, t1, G);
  OTAMD_CHECK_LAUNCH();
  af_apply_kernel<TP, TG, FORM><<<ns, AF_THREADS, 0, stream>>>((TP*)p, (const TG*)g, (bf16_t*)w, state, scratch, scal,
                                                               tensors, slabs, s0, G, clip_coef, sr, seed);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// One Adafactor step over the tensors [t_begin, t_end) of the table and their slabs [s_begin, s_end) (the whole
// tables for a store step; one tensor and its slabs for step_parameter).  form 0: p, g bf16; 1: p, g fp32;
// 2: p fp32 master, g bf16, w16 the bf16 working copy.  state: the fp32 state buffer; scratch: fp32 partials;
// slab_sq: double[2 * slabs]; scal: float[4 * tensors] (rms(p), rms(u) per tensor).  The tables are device
// arrays built by the host once (util/optimizer/adafactor_fused.py checks every range they name).
OTAMD_API int otamd_adafactor_step(void* p, const void* g, void* w16, int form, float* state, float* scratch,
                                   double* slab_sq, float* scal, const void* tensors, int t_begin, int t_end,
                                   const void* slabs, int s_begin, int s_end, const AdafactorGroup* groups,
                                   int n_groups, const float* clip_coef, int stochastic_rounding,
                                   unsigned long long seed, hipStream_t stream) {
  if (!p || !g || !state || !scratch || !slab_sq || !scal || !tensors || !slabs || !groups || !fs_form_ok(form, w16) ||
      !fs_group_count_ok(n_groups) || t_begin < 0 || t_end < t_begin || s_begin < 0 || s_end < s_begin)
    return OTAMD_EINVAL;
  if (!fs_aligned16(p, g, w16, state, scratch)) return OTAMD_EINVAL;
  if (t_end == t_begin || s_end == s_begin) return OTAMD_OK;
  const AdafactorGroups G = fs_groups_arg<AdafactorGroups>(groups, n_groups);
  return fs_dispatch(form, [&](auto F) {
    return af_launch<typename decltype(F)::TP, typename decltype(F)::TG, F.form>(
        p, g, F.w(w16), state, scratch, slab_sq, scal, (const AdafactorTensor*)tensors, t_begin, t_end,
        (const AdafactorSlab*)slabs, s_begin, s_end, G, clip_coef, F.sr(stochastic_rounding), seed, stream);
  });
}
