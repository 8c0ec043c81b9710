// What the factored optimizers (adafactor.hip, came.hip) share beyond flat_store.h: the tensor and slab tables, the
// EMA, torch's rsqrt, the fixed-order block sum, and, each written once here:
//   af_walk          every 8-aligned vector of a slab with its rsqrt factors (af_unorm_kernel and the apply kernels)
//   af_unorm_kernel  sum u^2 per slab, one template that each file instantiates under its own tag
// The masked 16-byte loads and stores, the pending-clip rounding and the parameter write of the apply kernels
// (fs_write_params) are flat_store.h's.  The statistics kernels stay in the two .hip files.  adafactor.hip's header
// comment describes the layout and the modes.
#pragma once
#include "flat_store.h"

#define AF_STAGE 4096   // floats of one LDS stage
#define AF_CT 4080      // widest column tile: its padded row (width + up to 15 floats of alignment) fits a stage
#define AF_THREADS 256

struct AdafactorTensor {
  long long offset, numel;                  // element range in the flat store
  long long row_off, col_off, full_off;     // fp32 state buffer: exp_avg_sq_row / _col (factored), exp_avg_sq
  long long rpart_off, cpart_off, rmean_off;   // fp32 scratch: mode 2 row / column partial sums; row-state mean per matrix
  int batch, rows, cols;
  int mode;
  int group;
  int slab_rows;   // mode 2: rows per slab; mode 1: matrices per stage
  int row_slabs;   // mode 2: slabs per matrix along the rows
  int col_tiles;   // mode 2: column tiles per row
  int slab0, n_slabs;   // this tensor's entries of the slab table
  int pad0, pad1;
};
struct AdafactorSlab {
  long long row0, row1;   // global rows b * rows + r (mode 1: whole matrices); mode 0: element range in the tensor
  int tensor;
  int col0, col1;
  int pad;
};

__device__ __forceinline__ float af_rsqrt(float x) { return 1.f / sqrtf(x); }   // torch's CPU rsqrt

// block sum of one double in a fixed order; red: 4 doubles
__device__ __forceinline__ double af_block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// state.mul_(beta).add_(mean, alpha=1 - beta)
__device__ __forceinline__ float af_ema(float state, float mean, float beta, float omb) {
  return fmaf(mean, omb, state * beta);
}

// ---- the walk: every 8-aligned vector of a slab with its gradient and factors -----------------------------------
// body(v, g, fac, valid): v = store element index of the vector, g = clipped gradients, fac = rsqrt factors,
// valid = lane mask of the elements that belong to the slab
template <typename TG, bool BFROUND, typename F>
__device__ __forceinline__ void af_walk(const TG* __restrict__ Gr, const float* __restrict__ state,
                                        const float* __restrict__ scratch, const AdafactorTensor& T,
                                        const AdafactorSlab& sl, float coef, bool clip, float* s_r, float* s_c,
                                        F&& body) {
  const int tid = threadIdx.x;
  if (T.mode == 0) {
    const long long e0 = T.offset + sl.row0, e1 = T.offset + sl.row1;
    for (long long v = (e0 & ~7LL) + 8 * tid; v < e1; v += 8 * AF_THREADS) {
      float g[8], fac[8];
      fs_load8<TG>(Gr, v, g);
      unsigned valid = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = v + j >= e0 && v + j < e1;
        g[j] = fs_clip<BFROUND>(g[j], coef, clip);
        fac[j] = ok ? af_rsqrt(state[T.full_off + (v + j - T.offset)]) : 0.f;
        valid |= ok ? 1u << j : 0u;
      }
      body(v, g, fac, valid);
    }
  } else if (T.mode == 1) {
    const int rc = T.rows * T.cols, mps = T.slab_rows;
    const long long m_begin = sl.row0 / T.rows, m_end = sl.row1 / T.rows;
    for (long long ms = m_begin; ms < m_end; ms += mps) {
      const int nm = (int)(m_end - ms < mps ? m_end - ms : mps);
      const long long e0 = T.offset + ms * rc, e1 = e0 + (long long)nm * rc;
      __syncthreads();
      for (int i = tid; i < nm * T.rows; i += AF_THREADS)
        s_r[i] = af_rsqrt(state[T.row_off + ms * T.rows + i] / scratch[T.rmean_off + ms + i / T.rows]);
      for (int i = tid; i < nm * T.cols; i += AF_THREADS) s_c[i] = af_rsqrt(state[T.col_off + ms * T.cols + i]);
      __syncthreads();
      for (long long v = (e0 & ~7LL) + 8 * tid; v < e1; v += 8 * AF_THREADS) {
        float g[8], fac[8];
        fs_load8<TG>(Gr, v, g);
        const int j0 = v < e0 ? (int)(e0 - v) : 0;
        const int li = (int)(v + j0 - e0);
        int ml = li / rc;
        const int rem = li - ml * rc;
        int r = rem / T.cols;
        int c = rem - r * T.cols;
        unsigned valid = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          g[j] = fs_clip<BFROUND>(g[j], coef, clip);
          fac[j] = 0.f;
          if (j >= j0 && v + j < e1) {
            fac[j] = s_r[ml * T.rows + r] * s_c[ml * T.cols + c];
            valid |= 1u << j;
            if (++c == T.cols) {
              c = 0;
              if (++r == T.rows) { r = 0; ++ml; }
            }
          }
        }
        body(v, g, fac, valid);
      }
    }
  } else {
    const int width = sl.col1 - sl.col0;
    const int vpr = (width + 7) / 8 + 1;
    const long long b = sl.row0 / T.rows;
    const int nrows = (int)(sl.row1 - sl.row0);   // <= 8 stages of rows <= 2048
    const float rmean = scratch[T.rmean_off + b];
    for (int c = tid; c < width; c += AF_THREADS) s_c[c] = af_rsqrt(state[T.col_off + b * T.cols + sl.col0 + c]);
    for (int i = tid; i < nrows; i += AF_THREADS) s_r[i] = af_rsqrt(state[T.row_off + sl.row0 + i] / rmean);
    __syncthreads();
    for (int q = tid; q < nrows * vpr; q += AF_THREADS) {
      const int i = q / vpr, j = q - i * vpr;
      const long long e0 = T.offset + (sl.row0 + i) * T.cols + sl.col0, e1 = e0 + width;
      const long long v = (e0 & ~7LL) + 8 * j;
      if (v >= e1) continue;
      float g[8], fac[8];
      fs_load8<TG>(Gr, v, g);
      unsigned valid = 0;
      const float rf = s_r[i];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const bool ok = v + jj >= e0 && v + jj < e1;
        g[jj] = fs_clip<BFROUND>(g[jj], coef, clip);
        fac[jj] = ok ? rf * s_c[v + jj - e0] : 0.f;
        valid |= ok ? 1u << jj : 0u;
      }
      body(v, g, fac, valid);
    }
  }
}

// ---- sum u^2 per slab, u recomputed from g and the fresh states: slab_sq[stride * slab + slot] ---------------------
// OWNER: a type of the including file (its group struct), so that each .hip registers a kernel of its own name
template <typename OWNER, typename TG, bool BFROUND>
__global__ void __launch_bounds__(AF_THREADS) af_unorm_kernel(const TG* __restrict__ Gr, const float* __restrict__ state,
                                                              const float* __restrict__ scratch,
                                                              double* __restrict__ slab_sq, int stride, int slot,
                                                              const AdafactorTensor* __restrict__ tensors,
                                                              const AdafactorSlab* __restrict__ slabs, int s0,
                                                              const float* __restrict__ clip_coef) {
  __shared__ float s_r[AF_STAGE];
  __shared__ float s_c[AF_STAGE];
  __shared__ double s_red[4];
  const int si = s0 + blockIdx.x;
  const AdafactorSlab sl = slabs[si];
  const AdafactorTensor T = tensors[sl.tensor];
  const bool clip = clip_coef != nullptr;
  const float coef = clip ? clip_coef[0] : 1.f;
  double acc = 0.0;
  af_walk<TG, BFROUND>(Gr, state, scratch, T, sl, coef, clip, s_r, s_c,
                       [&](long long, const float* g, const float* fac, unsigned valid) {
                         float s = 0.f;
#pragma unroll
                         for (int j = 0; j < 8; ++j) {
                           const float u = fac[j] * g[j];
                           if (valid >> j & 1) s = fmaf(u, u, s);
                         }
                         acc += (double)s;
                       });
  const double t = af_block_sum_d(acc, s_red);
  if (threadIdx.x == 0) slab_sq[stride * (long long)si + slot] = t;
}
