// Fused CAME (confidence-guided adaptive memory-efficient optimization) over a flat parameter store.  Replaces,
// per parameter tensor, the reference's
//   modules/util/optimizer/CAME.py:79-178  (CAME.step_parameter)
// built at modules/util/create.py:938-951, with NINE launches over the whole store (seven when no matrix spans
// slabs; the reference runs ~35 torch ops per tensor per step in a Python loop):
//   1 stats     row / column sums of g^2 + eps1 per slab; states that a slab owns whole (unfactored tensors,
//               matrices that fit one LDS stage) take their beta2 EMA here
//   2 fold sq   matrices that span slabs: a thread per row / per column sums its partials in slab order, EMA
//   3 rmean sq  those matrices: mean of the fresh row states, a workgroup per matrix
//   4 unorm     sum u^2 per slab, u = rsqrt(row / mean(row)) rsqrt(col) g recomputed (never materialised)
//   5 scalars   per tensor: slab sums folded in slab order -> rms(u)
//   6 moment    u_c = u / max(rms(u) / clip_threshold, 1);  m = beta1 m + (1 - beta1) u_c (written);  row / column
//               sums of (u_c - m)^2 + eps2 per slab, with the beta3 EMA where a slab owns the state whole
//   7 fold res  as 2 with beta3, on the instability states
//   8 rmean res as 3
//   9 apply     update = rsqrt(res_row / mean(res_row)) rsqrt(res_col) m (m itself for unfactored tensors), weight
//               decay, parameter write (bf16 RNE or stochastic, fp32, fp32 master + bf16 working copy)
// Every reduction has a fixed order (no atomics): two runs give the same bits.
//
// Shared with adafactor.hip, in adafactor_walk.h: the unorm kernel of pass 4, the slab walk of pass 9, the EMA; with
// every flat-store optimizer, in flat_store.h: the masked loads and stores and the parameter write of pass 9.  The
// statistics kernel of passes 1 and 6 restates af_stats_kernel's
// three-mode body (sharing it cost 0.4 ms a step through code placement).
//
// Tables.  The Adafactor tensor and slab tables, unchanged (adafactor_walk.h; adafactor.hip describes the three
// modes).  The second-moment and the instability factors live in two fp32 state buffers indexed by the same
// row_off / col_off (full_off is used in the first only), their partial sums and row-state means in two scratch
// buffers indexed by the same rpart_off / cpart_off / rmean_off.  The first moment m is fp32, full-size, indexed by
// store offset.  The fold table (CameFold) spreads the folds of the mode 2 tensors over workgroups: an entry is
// AF_THREADS consecutive rows, or columns, of one tensor (kind 0 / 1; every thread owns one and adds its partials
// in slab order, the order a serial fold uses), or one matrix whose row-state mean is due (kind 2).
//
// Traffic, bytes per parameter (bf16 store / fp32 store / master): stats g 2/4/2, unorm g 2/4/2, moment g + m
// read + m written 10/12/10, apply m + p read + p written 8/12/14 -> 22 / 32 / 28.  m is written in pass 6 and
// read back in pass 9; recomputing it there instead would need both factor sets in LDS at once.
//
// Arithmetic: fp32 element ops in the reference's order (-ffp-contract=off; the fused multiply-adds are the
// ones torch's CPU add_(alpha=) kernels use), fp32 sums.  tests/_oracle_came.py restates it.
#include "adafactor_walk.h"

struct CameGroup {
  float lr;
  float alpha_wd;            // -weight_decay * lr rounded once; 0: no decay
  float eps1, eps2, clip_threshold;
  float beta1, one_minus_beta1;   // first moment
  float beta2, one_minus_beta2;   // second-moment factors
  float beta3, one_minus_beta3;   // instability factors
  int pad;
};
struct CameGroups { CameGroup g[FS_MAX_GROUPS]; };
struct CameFold {
  long long i0, i1;   // kind 0: global rows b * rows + r; kind 1: global columns b * cols + c; kind 2: matrices
  int tensor;
  int kind;
};

// ---- 1 and 6: statistics ------------------------------------------------------------------------------------------
// PASS 0: x = g, statistic x^2 + eps1, beta2, written to the second-moment buffers (state, scratch).
// PASS 1: x = u_c - m with the new m (written to M), statistic x^2 + eps2, beta3, written to the instability
//         buffers; u's factors come from the second-moment buffers (fstate, fscratch), rms(u) from scal.
// The sums run in af_stats_kernel's order: the second-moment states carry Adafactor's bits.
template <typename TG, bool BFROUND, int PASS>
__global__ void __launch_bounds__(AF_THREADS) came_stats_kernel(const TG* __restrict__ Gr, float* __restrict__ M,
                                                                const float* __restrict__ fstate,
                                                                const float* __restrict__ fscratch,
                                                                float* __restrict__ state, float* __restrict__ scratch,
                                                                const float* __restrict__ scal,
                                                                const AdafactorTensor* __restrict__ tensors,
                                                                const AdafactorSlab* __restrict__ slabs, int s0,
                                                                CameGroups groups,
                                                                const float* __restrict__ clip_coef) {
  __shared__ __attribute__((aligned(16))) float s_stage[AF_STAGE + 16];
  // mode 1: row factors while a stage is filled (pass 1), then the stage's fresh row states; mode 2: column sums
  __shared__ float s_acc[AF_STAGE];
  __shared__ float s_c[PASS == 1 ? AF_STAGE : 1];   // pass 1: column factors
  const int tid = threadIdx.x;
  const int si = s0 + blockIdx.x;
  const AdafactorSlab sl = slabs[si];
  const AdafactorTensor T = tensors[sl.tensor];
  const CameGroup G = groups.g[T.group];
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  const float eps = PASS == 0 ? G.eps1 : G.eps2;
  const float beta = PASS == 0 ? G.beta2 : G.beta3, omb = PASS == 0 ? G.one_minus_beta2 : G.one_minus_beta3;
  // update.div_((rms(update) / clip_threshold).clamp_(min=1.0))
  float denom = 1.f;
  if constexpr (PASS == 1) denom = fmaxf(scal[sl.tensor] / G.clip_threshold, 1.f);
  // pass 1, one vector: x = u_c - m, m written
  auto moment = [&](long long v, const float* g, const float* fac, unsigned valid, float* x) {
    float m[8];
    fs_load8<float>(M, v, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float u = fac[j] * g[j];
      u = u / denom;
      m[j] = fmaf(u, G.one_minus_beta1, m[j] * G.beta1);   // exp_avg.mul_(beta1).add_(update, alpha=1 - beta1)
      x[j] = u - m[j];
    }
    fs_store8(M, v, m, valid);
  };

  if (T.mode == 0) {
    for (long long i = sl.row0 + tid; i < sl.row1; i += AF_THREADS) {
      const float g = fs_clip<BFROUND>(fs_load1<TG>(Gr, T.offset + i), coef, clip);
      if constexpr (PASS == 0) {
        float* v = state + T.full_off + i;
        *v = af_ema(*v, g * g + eps, beta, omb);
      } else {   // no instability state: the update is m
        float u = af_rsqrt(fstate[T.full_off + i]) * g;
        u = u / denom;
        float* m = M + T.offset + i;
        *m = fmaf(u, G.one_minus_beta1, *m * G.beta1);
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
      if constexpr (PASS == 1) {
        for (int i = tid; i < nm * T.rows; i += AF_THREADS)
          s_acc[i] = af_rsqrt(fstate[T.row_off + ms * T.rows + i] / fscratch[T.rmean_off + ms + i / T.rows]);
        for (int i = tid; i < nm * T.cols; i += AF_THREADS) s_c[i] = af_rsqrt(fstate[T.col_off + ms * T.cols + i]);
        __syncthreads();
      }
      for (long long v = a0 + 8 * tid; v < e1; v += 8 * AF_THREADS) {
        float f[8];
        fs_load8<TG>(Gr, v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = fs_clip<BFROUND>(f[j], coef, clip);
        if constexpr (PASS == 1) {
          float fac[8], x[8];
          const int j0 = v < e0 ? (int)(e0 - v) : 0;
          const int li = (int)(v + j0 - e0);
          int ml = li / rc;
          const int rem = li - ml * rc;
          int r = rem / T.cols;
          int c = rem - r * T.cols;
          unsigned valid = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            fac[j] = 0.f;
            if (j >= j0 && v + j < e1) {
              fac[j] = s_acc[ml * T.rows + r] * s_c[ml * T.cols + c];
              valid |= 1u << j;
              if (++c == T.cols) {
                c = 0;
                if (++r == T.rows) { r = 0; ++ml; }
              }
            }
          }
          moment(v, f, fac, valid, x);
#pragma unroll
          for (int j = 0; j < 8; ++j) s_stage[v - a0 + j] = x[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) s_stage[v - a0 + j] = f[j];
        }
      }
      __syncthreads();
      const int nrows = nm * T.rows, ncols = nm * T.cols;
      for (int i = tid; i < nrows; i += AF_THREADS) {   // row i of the stage: elements [i * cols, (i + 1) * cols)
        const float* x = s_stage + sh + (long long)i * T.cols;
        float s = 0.f;
        for (int c = 0; c < T.cols; ++c) s += x[c] * x[c] + eps;
        float* rs = state + T.row_off + ms * T.rows + i;
        const float nv = af_ema(*rs, s / (float)T.cols, beta, omb);
        *rs = nv;
        s_acc[i] = nv;
      }
      for (int i = tid; i < ncols; i += AF_THREADS) {
        const int ml = i / T.cols, c = i - ml * T.cols;
        const float* x = s_stage + sh + ml * rc + c;
        float s = 0.f;
        for (int r = 0; r < T.rows; ++r) {
          const float g = x[r * T.cols];
          s += g * g + eps;
        }
        float* cs = state + T.col_off + ms * T.cols + i;
        *cs = af_ema(*cs, s / (float)T.rows, beta, omb);
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
    float rmean = 1.f;
    if constexpr (PASS == 1) {
      rmean = fscratch[T.rmean_off + b];
      for (int c = tid; c < width; c += AF_THREADS) s_c[c] = af_rsqrt(fstate[T.col_off + b * T.cols + sl.col0 + c]);
    }
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
          for (int jj = 0; jj < 8; ++jj) f[jj] = fs_clip<BFROUND>(f[jj], coef, clip);
          if constexpr (PASS == 1) {
            float fac[8], x[8];
            const float rf = af_rsqrt(fstate[T.row_off + r0 + i] / rmean);
            unsigned valid = 0;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              const bool ok = v + jj >= e0 && v + jj < e1;
              fac[jj] = ok ? rf * s_c[v + jj - e0] : 0.f;
              valid |= ok ? 1u << jj : 0u;
            }
            moment(v, f, fac, valid, x);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) s_stage[i * W8 + 8 * j + jj] = x[jj];
          } else {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) s_stage[i * W8 + 8 * j + jj] = f[jj];
          }
        }
      }
      __syncthreads();
      const int wave = tid >> 6, lane = tid & 63;
      for (int i = wave; i < nr; i += AF_THREADS / 64) {   // row sums over this tile's columns: a wave per row
        const int sh = (int)((T.offset + (r0 + i) * T.cols + sl.col0) & 7);
        const float* x = s_stage + i * W8 + sh;
        float s = 0.f;
        for (int c = lane; c < width; c += 64) s += x[c] * x[c] + eps;
        s = wave_sum(s);
        if (lane == 0) scratch[T.rpart_off + (r0 + i) * T.col_tiles + tile] = s;
      }
      for (int c = tid; c < width; c += AF_THREADS) {      // column sums over the stage's rows: a thread per column
        float s = 0.f;
        for (int i = 0; i < nr; ++i) {
          const int sh = (int)((T.offset + (r0 + i) * T.cols + sl.col0) & 7);
          const float g = s_stage[i * W8 + sh + c];
          s += g * g + eps;
        }
        s_acc[c] += s;   // each thread owns its columns
      }
    }
    const long long sidx = (sl.row0 - b * T.rows) / T.slab_rows;
    for (int c = tid; c < width; c += AF_THREADS)
      scratch[T.cpart_off + (b * T.row_slabs + sidx) * T.cols + sl.col0 + c] = s_acc[c];
  }
}

// ---- 2 and 7: fold the partials of the matrices that span slabs, a thread per row / per column -----------------
__global__ void __launch_bounds__(AF_THREADS) came_fold_kernel(float* __restrict__ state,
                                                               const float* __restrict__ scratch,
                                                               const AdafactorTensor* __restrict__ tensors,
                                                               const CameFold* __restrict__ fold, int f0,
                                                               CameGroups groups, int pass) {
  const CameFold f = fold[f0 + blockIdx.x];
  const long long i = f.i0 + threadIdx.x;
  if (i >= f.i1) return;
  const AdafactorTensor T = tensors[f.tensor];
  const CameGroup G = groups.g[T.group];
  const float beta = pass == 0 ? G.beta2 : G.beta3, omb = pass == 0 ? G.one_minus_beta2 : G.one_minus_beta3;
  if (f.kind == 0) {
    float s = 0.f;
    for (int j = 0; j < T.col_tiles; ++j) s += scratch[T.rpart_off + i * T.col_tiles + j];
    float* rs = state + T.row_off + i;
    *rs = af_ema(*rs, s / (float)T.cols, beta, omb);
  } else {
    const long long b = i / T.cols;
    const int c = (int)(i - b * T.cols);
    float s = 0.f;
    for (int k = 0; k < T.row_slabs; ++k) s += scratch[T.cpart_off + (b * T.row_slabs + k) * T.cols + c];
    float* cs = state + T.col_off + i;
    *cs = af_ema(*cs, s / (float)T.rows, beta, omb);
  }
}

// ---- 3 and 8: mean of the fresh row states of a matrix that spans slabs, a workgroup per matrix ----------------
__global__ void __launch_bounds__(AF_THREADS) came_rmean_kernel(const float* __restrict__ state,
                                                                float* __restrict__ scratch,
                                                                const AdafactorTensor* __restrict__ tensors,
                                                                const CameFold* __restrict__ fold, int f0) {
  __shared__ float red[AF_THREADS / 64];
  const CameFold f = fold[f0 + blockIdx.x];
  const AdafactorTensor T = tensors[f.tensor];
  const long long b = f.i0;
  float s = 0.f;
  for (int r = threadIdx.x; r < T.rows; r += AF_THREADS) s += state[T.row_off + b * T.rows + r];
  const float t = block_sum(s, red);
  if (threadIdx.x == 0) scratch[T.rmean_off + b] = t / (float)T.rows;
}

// ---- 4: sum u^2 per slab: af_unorm_kernel<CameGroup, ...> (adafactor_walk.h) -> slab_sq[s] ----------------------

// ---- 5: per-tensor scalars: the slab sums in slab order -> scal[t] = rms(u) ------------------------------------
__global__ void came_scalars_kernel(const double* __restrict__ slab_sq, float* __restrict__ scal,
                                    const AdafactorTensor* __restrict__ tensors, int t0, int t1) {
  const int t = t0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= t1) return;
  const AdafactorTensor T = tensors[t];
  double su = 0.0;
  for (int s = T.slab0; s < T.slab0 + T.n_slabs; ++s) su += slab_sq[s];
  scal[t] = (float)sqrt(su) / (float)sqrt((double)T.numel);   // tensor.norm(2) / numel ** 0.5
}

// ---- 9: apply ---------------------------------------------------------------------------------------------------
// FORM 0: bf16 store (RNE or stochastic); 1: fp32 store; 2: fp32 master + bf16 working copy W = rne(master)
template <typename TP, int FORM>
__global__ void __launch_bounds__(AF_THREADS) came_apply_kernel(TP* __restrict__ P, const float* __restrict__ M,
                                                                bf16_t* __restrict__ W,
                                                                const float* __restrict__ state,
                                                                const float* __restrict__ scratch,
                                                                const AdafactorTensor* __restrict__ tensors,
                                                                const AdafactorSlab* __restrict__ slabs, int s0,
                                                                CameGroups groups, int sr, unsigned long long seed) {
  __shared__ float s_r[AF_STAGE];
  __shared__ float s_c[AF_STAGE];
  const AdafactorSlab sl = slabs[s0 + blockIdx.x];
  const AdafactorTensor T = tensors[sl.tensor];
  const CameGroup G = groups.g[T.group];
  const uint32_t k = fs_seed_key(seed);
  const float lr = G.lr, alpha = G.alpha_wd;
  const bool decay = alpha != 0.f;
  // m: the new first moment; fac: the instability factors (1 for unfactored tensors)
  auto body = [&](long long v, const float* m, const float* fac, unsigned valid) {
    float p[8];
    fs_load8<TP>(P, v, p);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float u = fac[j] * m[j];   // res_approx.mul_(exp_avg)
      u = u * lr;                // update.mul_(lr)
      float x = p[j];
      if (decay) {
        x = fmaf(x, alpha, x);   // p.add_(p, alpha=-weight_decay * lr): a bf16 result without stochastic rounding
        if constexpr (FORM == 0)
          if (!sr) x = rbf(x);
      }
      p[j] = x - u;              // p.add_(-update)
    }
    fs_write_params<FORM>(P, W, v, p, valid, sr, k);
  };
  if (T.mode == 0) {   // update = exp_avg
    const long long e0 = T.offset + sl.row0, e1 = T.offset + sl.row1;
    for (long long v = (e0 & ~7LL) + 8 * threadIdx.x; v < e1; v += 8 * AF_THREADS) {
      float m[8], fac[8];
      fs_load8<float>(M, v, m);
      unsigned valid = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        fac[j] = 1.f;
        valid |= (v + j >= e0 && v + j < e1) ? 1u << j : 0u;
      }
      body(v, m, fac, valid);
    }
  } else {
    af_walk<float, false>(M, state, scratch, T, sl, 1.f, false, s_r, s_c, body);
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_came_group_size(void) { return (int)sizeof(CameGroup); }
OTAMD_API int otamd_came_fold_size(void) { return (int)sizeof(CameFold); }

namespace {
struct CameArgs {
  void* p;
  const void* g;
  void* w;
  float *m, *state_sq, *state_res, *scratch_sq, *scratch_res;
  double* slab_sq;
  float* scal;
  const AdafactorTensor* tensors;
  const AdafactorSlab* slabs;
  const CameFold* fold;
  int t0, t1, s0, s1, f0, f1, r0, r1;
  const float* clip_coef;
  int sr;
  unsigned long long seed;
};
}   // namespace

template <typename TP, typename TG, int FORM>
static int came_launch(const CameArgs& a, const CameGroups& G, hipStream_t stream) {
  const int ns = a.s1 - a.s0, nt = a.t1 - a.t0, nf = a.f1 - a.f0, nr = a.r1 - a.r0;
  const TG* g = (const TG*)a.g;
  came_stats_kernel<TG, FORM == 0, 0><<<ns, AF_THREADS, 0, stream>>>(g, nullptr, nullptr, nullptr, a.state_sq, a.scratch_sq,
                                                                     nullptr, a.tensors, a.slabs, a.s0, G, a.clip_coef);
  OTAMD_CHECK_LAUNCH();
  if (nf > 0) {
    came_fold_kernel<<<nf, AF_THREADS, 0, stream>>>(a.state_sq, a.scratch_sq, a.tensors, a.fold, a.f0, G, 0);
    OTAMD_CHECK_LAUNCH();
  }
  if (nr > 0) {
    came_rmean_kernel<<<nr, AF_THREADS, 0, stream>>>(a.state_sq, a.scratch_sq, a.tensors, a.fold, a.r0);
    OTAMD_CHECK_LAUNCH();
  }
  af_unorm_kernel<CameGroup, TG, FORM == 0><<<ns, AF_THREADS, 0, stream>>>(g, a.state_sq, a.scratch_sq, a.slab_sq, 1, 0,
                                                                           a.tensors, a.slabs, a.s0, a.clip_coef);
  OTAMD_CHECK_LAUNCH();
  came_scalars_kernel<<<(nt + 255) / 256, 256, 0, stream>>>(a.slab_sq, a.scal, a.tensors, a.t0, a.t1);
  OTAMD_CHECK_LAUNCH();
  came_stats_kernel<TG, FORM == 0, 1><<<ns, AF_THREADS, 0, stream>>>(g, a.m, a.state_sq, a.scratch_sq, a.state_res,
                                                                     a.scratch_res, a.scal, a.tensors, a.slabs, a.s0, G,
                                                                     a.clip_coef);
  OTAMD_CHECK_LAUNCH();
  if (nf > 0) {
    came_fold_kernel<<<nf, AF_THREADS, 0, stream>>>(a.state_res, a.scratch_res, a.tensors, a.fold, a.f0, G, 1);
    OTAMD_CHECK_LAUNCH();
  }
  if (nr > 0) {
    came_rmean_kernel<<<nr, AF_THREADS, 0, stream>>>(a.state_res, a.scratch_res, a.tensors, a.fold, a.r0);
    OTAMD_CHECK_LAUNCH();
  }
  came_apply_kernel<TP, FORM><<<ns, AF_THREADS, 0, stream>>>((TP*)a.p, a.m, (bf16_t*)a.w, a.state_res, a.scratch_res,
                                                             a.tensors, a.slabs, a.s0, G, a.sr, a.seed);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// One CAME step over the tensors [t_begin, t_end) of the table, their slabs [s_begin, s_end), their fold entries
// [f_begin, f_end) (kinds 0 and 1) and their row-mean entries [r_begin, r_end) (kind 2) (the whole tables for a
// store step; one tensor's ranges for step_parameter).  form 0: p, g bf16; 1: p, g fp32; 2: p fp32 master, g
// bf16, w16 the bf16 working copy.  m: the fp32 first moment, indexed as the store.  state_sq / state_res: the
// fp32 second-moment and instability states; scratch_sq / scratch_res: their fp32 partials; slab_sq:
// double[slabs]; scal: float[tensors] (rms(u)).  The tables are device arrays built by the host once
// (util/optimizer/came_fused.py checks every range they name).
OTAMD_API int otamd_came_step(void* p, const void* g, void* w16, int form, float* m, float* state_sq, float* state_res,
                              float* scratch_sq, float* scratch_res, double* slab_sq, float* scal, const void* tensors,
                              int t_begin, int t_end, const void* slabs, int s_begin, int s_end, const void* fold,
                              int f_begin, int f_end, int r_begin, int r_end, const CameGroup* groups, int n_groups,
                              const float* clip_coef, int stochastic_rounding, unsigned long long seed,
                              hipStream_t stream) {
  if (!p || !g || !m || !state_sq || !state_res || !scratch_sq || !scratch_res || !slab_sq || !scal || !tensors ||
      !slabs || !fold || !groups || !fs_form_ok(form, w16) || !fs_group_count_ok(n_groups) || t_begin < 0 ||
      t_end < t_begin || s_begin < 0 || s_end < s_begin || f_begin < 0 || f_end < f_begin || r_begin < 0 ||
      r_end < r_begin)
    return OTAMD_EINVAL;
  if (!fs_aligned16(p, g, w16, m, state_sq, state_res, scratch_sq, scratch_res)) return OTAMD_EINVAL;
  if (t_end == t_begin || s_end == s_begin) return OTAMD_OK;
  const CameGroups G = fs_groups_arg<CameGroups>(groups, n_groups);
  return fs_dispatch(form, [&](auto F) {
    const CameArgs a = {p, g, F.w(w16), m, state_sq, state_res, scratch_sq, scratch_res, slab_sq, scal,
                        (const AdafactorTensor*)tensors, (const AdafactorSlab*)slabs, (const CameFold*)fold,
                        t_begin, t_end, s_begin, s_end, f_begin, f_end, r_begin, r_end, clip_coef,
                        F.sr(stochastic_rounding), seed};
    return came_launch<typename decltype(F)::TP, typename decltype(F)::TG, F.form>(a, G, stream);
  });
}
