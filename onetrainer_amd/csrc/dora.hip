// DoRA (weight-decomposed LoRA) on a frozen base: merge and gradient projection.  Replaces, per adapted Linear / Conv2d,
// the reference's
//   modules/module/LoRAModule.py:385-419  (DoRAModule.forward: WP = W + (alpha/rank) B A, norm over every axis but
//                                          one (detached) + eps, W' = dora_scale * (WP / norm), op(x, W', bias))
// and the autograd of that expression.  The model runs the plain base graph on W'; its weight-gradient GEMMs leave
// dL/dW' in a bf16 buffer G of the same layout, and the projection turns G into the fp32 gradients of lora_down,
// lora_up and dora_scale with the norm held constant, as the reference does.
//
// Every weight is a matrix [out, K], K = kk * cin, in store layout (conv: [out][kh][kw][cin], so column
// c = (kh * k + kw) * cin + ci); down is [rank, K], up is [out, rank], all adapters fp32.  Weff = W + s up down is
// formed on the fly in fp32 from a 64 x 64 tile of W and the matching up / down tiles in LDS; a full-size fp32 Weff
// never exists.  A workgroup owns whole reduction lines -- 64 input channels (every row, every kernel tap) for the
// input axis, 64 rows for the output axis -- so every sum has a fixed order (a thread's partial over its rows or
// columns ascending, then the 16 thread partials ascending) and needs no atomics: two runs give the same bits.
//
//   merge    pass 1: n = sqrt(sum Weff^2) + eps;  pass 2: W' = bf16_rne(scale * (Weff / n)), 0 where n == 0
//   project  column owner: d_down = s up^T H (and d_scale on the input axis)
//            row owner:    d_up = s H down^T (and d_scale on the output axis)
//            with H = (G * scale) / n and d_scale = sum G * (Weff / n), both 0 where n == 0 (a zero-padded input
//            channel of conv_in with eps off)
// All launches are table-driven (DoraEntry per adapted module); the merge serves every module in one launch, the
// projection a range of entries (one base GEMM's modules) per call.  The fp32 products are VALU FMAs (rank <= 64).
#include "common.h"

#include <algorithm>

#define DR_T 64      // tile edge (rows and columns)
#define DR_LD 68     // LDS row stride in floats: 16-byte aligned rows, rows 4 banks apart
#define DR_RMAX 64   // largest rank (two DR_RMAX x DR_LD fp32 tiles in LDS)

struct DoraEntry {
  long long w_off;                          // W, elements into the bf16 base store
  long long wp_off;                         // W' and G, elements into their bf16 buffers
  long long down_off, up_off, scale_off;    // elements into the fp32 adapter store (values and gradients alike)
  long long norm_off;                       // n, elements into the fp32 norm buffer
  int out, cin, kk, rank;
  int cblk0, rblk0;                         // first workgroup of this entry in the column-owner / row-owner grids
  float s;                                  // alpha / rank
  int pad;
};

__device__ __forceinline__ float4v dr_ld_bf4(const bf16_t* p) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const u2 x = *reinterpret_cast<const u2*>(p);
  float4v r;
  r.x = __uint_as_float(x.x << 16); r.y = __uint_as_float(x.x & 0xffff0000u);
  r.z = __uint_as_float(x.y << 16); r.w = __uint_as_float(x.y & 0xffff0000u);
  return r;
}
__device__ __forceinline__ void dr_st_bf4(bf16_t* p, const float* f) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  u2 y;
  y.x = (uint32_t)f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16);
  y.y = (uint32_t)f2bf(f[2]) | ((uint32_t)f2bf(f[3]) << 16);
  *reinterpret_cast<u2*>(p) = y;
}

// sU[j][row] = up[row0 + row][j] (0 past `out`)
__device__ __forceinline__ void dr_load_up(float (*sU)[DR_LD], const float* __restrict__ up, int row0, int out, int r) {
  for (int i = threadIdx.x; i < DR_T * r; i += 256) {
    const int row = i / r, j = i - row * r;
    sU[j][row] = row0 + row < out ? up[(long long)(row0 + row) * r + j] : 0.f;
  }
}
// sD[j][col] = down[j][c0 + col] (0 past `ncols`)
__device__ __forceinline__ void dr_load_down(float (*sD)[DR_LD], const float* __restrict__ down, long long K,
                                             long long c0, int ncols, int r) {
  for (int i = threadIdx.x; i < DR_T * r; i += 256) {
    const int j = i >> 6, col = i & 63;
    sD[j][col] = col < ncols ? down[(long long)j * K + c0 + col] : 0.f;
  }
}
// v[i][k] = sum_j up[ty*4+i][j] down[j][tx*4+k], j ascending
__device__ __forceinline__ void dr_tile_ba(const float (*sU)[DR_LD], const float (*sD)[DR_LD], int r, int tx, int ty,
                                           float v[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[i][k] = 0.f;
  for (int j = 0; j < r; ++j) {
    const float4v a = *reinterpret_cast<const float4v*>(&sU[j][ty * 4]);
    const float4v b = *reinterpret_cast<const float4v*>(&sD[j][tx * 4]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[i][k] = fmaf(a[i], b[k], v[i][k]);
  }
}

// the entry of [e0, e1) whose blocks hold workgroup `bid` of the column-owner (COLS) or row-owner grid
template <bool COLS>
__device__ __forceinline__ int dr_find(const DoraEntry* __restrict__ tab, int e0, int e1, int bid) {
  int lo = e0, hi = e1 - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((COLS ? tab[mid].cblk0 : tab[mid].rblk0) <= bid) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum over the 16 thread partials of each of the 64 lines, ascending; the result in sLine[0..63] (threads 0..63)
__device__ __forceinline__ float dr_line_sum(float (*sRed)[DR_T], int tid) {
  float t = 0.f;
  if (tid < DR_T)
    for (int p = 0; p < 16; ++p) t += sRed[p][tid];
  return t;
}

// ---- merge --------------------------------------------------------------------------------------------------------
// AXIS 0: the input-channel axis is kept (n and scale per ci; a workgroup owns 64 input channels);
// AXIS 1: the output-channel axis is kept (per row; a workgroup owns 64 rows)
template <int AXIS>
__global__ void __launch_bounds__(256) dora_merge_kernel(const DoraEntry* __restrict__ tab, int n_entries,
                                                         const bf16_t* __restrict__ W, const float* __restrict__ P,
                                                         float* __restrict__ norms, bf16_t* __restrict__ WP, float eps) {
  __shared__ __attribute__((aligned(16))) float sU[DR_RMAX][DR_LD];
  __shared__ __attribute__((aligned(16))) float sD[DR_RMAX][DR_LD];
  __shared__ float sRed[16][DR_T];
  __shared__ float sN[DR_T], sS[DR_T];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const DoraEntry e = tab[dr_find<AXIS == 0>(tab, 0, n_entries, blockIdx.x)];
  const int lb = blockIdx.x - (AXIS == 0 ? e.cblk0 : e.rblk0);
  const long long K = (long long)e.kk * e.cin;
  const int r = e.rank;
  const float* up = P + e.up_off;
  const float* down = P + e.down_off;
  const bf16_t* w = W + e.w_off;
  bf16_t* wp = WP + e.wp_off;
  float ss[4] = {0.f, 0.f, 0.f, 0.f};

  if (AXIS == 0) {
    const int ci0 = lb * DR_T, ncols = min(DR_T, e.cin - ci0);
    const bool cvalid = tx * 4 < ncols;
    for (int pass = 0; pass < 2; ++pass) {
      for (int g = 0; g < e.kk; ++g) {
        const long long c0 = (long long)g * e.cin + ci0;
        dr_load_down(sD, down, K, c0, ncols, r);
        for (int row0 = 0; row0 < e.out; row0 += DR_T) {
          dr_load_up(sU, up, row0, e.out, r);
          __syncthreads();
          float v[4][4];
          dr_tile_ba(sU, sD, r, tx, ty, v);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = row0 + ty * 4 + i;
            if (row < e.out && cvalid) {
              const long long at = (long long)row * K + c0 + tx * 4;
              const float4v w4 = dr_ld_bf4(w + at);
              float o[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const float x = w4[k] + e.s * v[i][k];
                if (pass == 0) {
                  ss[k] += x * x;
                } else {
                  const float nn = sN[tx * 4 + k];
                  o[k] = nn != 0.f ? sS[tx * 4 + k] * (x / nn) : 0.f;
                }
              }
              if (pass == 1) dr_st_bf4(wp + at, o);
            }
          }
          __syncthreads();
        }
      }
      if (pass == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sRed[ty][tx * 4 + k] = ss[k];
        __syncthreads();
        const float tot = dr_line_sum(sRed, tid);
        if (tid < DR_T) {
          const float nn = sqrtf(tot) + eps;
          sN[tid] = nn;
          sS[tid] = tid < ncols ? P[e.scale_off + ci0 + tid] : 0.f;
          if (tid < ncols) norms[e.norm_off + ci0 + tid] = nn;
        }
        __syncthreads();
      }
    }
  } else {
    const int row0 = lb * DR_T;
    dr_load_up(sU, up, row0, e.out, r);
    for (int pass = 0; pass < 2; ++pass) {
      for (long long c0 = 0; c0 < K; c0 += DR_T) {
        const int ncols = (int)min((long long)DR_T, K - c0);
        const bool cvalid = tx * 4 < ncols;
        dr_load_down(sD, down, K, c0, ncols, r);
        __syncthreads();
        float v[4][4];
        dr_tile_ba(sU, sD, r, tx, ty, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + ty * 4 + i;
          if (row < e.out && cvalid) {
            const long long at = (long long)row * K + c0 + tx * 4;
            const float4v w4 = dr_ld_bf4(w + at);
            float o[4];
            const float nn = pass ? sN[ty * 4 + i] : 1.f, sc = pass ? sS[ty * 4 + i] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float x = w4[k] + e.s * v[i][k];
              if (pass == 0) ss[i] += x * x;
              else o[k] = nn != 0.f ? sc * (x / nn) : 0.f;
            }
            if (pass == 1) dr_st_bf4(wp + at, o);
          }
        }
        __syncthreads();
      }
      if (pass == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sRed[tx][ty * 4 + i] = ss[i];
        __syncthreads();
        const float tot = dr_line_sum(sRed, tid);
        if (tid < DR_T) {
          const float nn = sqrtf(tot) + eps;
          const bool rv = row0 + tid < e.out;
          sN[tid] = nn;
          sS[tid] = rv ? P[e.scale_off + row0 + tid] : 0.f;
          if (rv) norms[e.norm_off + row0 + tid] = nn;
        }
        __syncthreads();
      }
    }
  }
}

// ---- projection ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dr_put(float* p, float v, int accumulate) { *p = accumulate ? *p + v : v; }

// column owner: 64 input channels of one entry, every kernel tap, every row.  d_down[j][c] = s sum_o up[o][j] H[o][c]
// (o ascending); AXIS 0 also d_scale[ci] = sum G (Weff / n)
template <int AXIS>
__global__ void __launch_bounds__(256) dora_project_cols_kernel(const DoraEntry* __restrict__ tab, int e0, int e1,
                                                                int blk_base, const bf16_t* __restrict__ W,
                                                                const float* __restrict__ P, float* __restrict__ dP,
                                                                const float* __restrict__ norms,
                                                                const bf16_t* __restrict__ G, int accumulate) {
  __shared__ __attribute__((aligned(16))) float sU[DR_RMAX][DR_LD];
  __shared__ __attribute__((aligned(16))) float sD[AXIS == 0 ? DR_RMAX : 1][DR_LD];
  __shared__ __attribute__((aligned(16))) float sH[DR_T][DR_LD];   // H tile [row][col]; reused for the line sums
  __shared__ float sN[DR_T], sS[DR_T];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, col = tid & 63, jg = tid >> 6;
  const int bid = blockIdx.x + blk_base;
  const DoraEntry e = tab[dr_find<true>(tab, e0, e1, bid)];
  const int lb = bid - e.cblk0;
  const long long K = (long long)e.kk * e.cin;
  const int r = e.rank;
  const int ci0 = lb * DR_T, ncols = min(DR_T, e.cin - ci0);
  const bool cvalid = tx * 4 < ncols;
  const float* up = P + e.up_off;
  const bf16_t* w = W + e.w_off;
  const bf16_t* gp = G + e.wp_off;
  float ds[4] = {0.f, 0.f, 0.f, 0.f};
  if (AXIS == 0) {
    if (tid < DR_T) {
      sN[tid] = tid < ncols ? norms[e.norm_off + ci0 + tid] : 0.f;
      sS[tid] = tid < ncols ? P[e.scale_off + ci0 + tid] : 0.f;
    }
  }
  for (int g = 0; g < e.kk; ++g) {
    const long long c0 = (long long)g * e.cin + ci0;
    if (AXIS == 0) dr_load_down(sD, P + e.down_off, K, c0, ncols, r);
    float acc[DR_RMAX / 4];
#pragma unroll
    for (int jj = 0; jj < DR_RMAX / 4; ++jj) acc[jj] = 0.f;
    for (int row0 = 0; row0 < e.out; row0 += DR_T) {
      dr_load_up(sU, up, row0, e.out, r);
      if (AXIS == 1 && tid < DR_T) {
        const bool rv = row0 + tid < e.out;
        sN[tid] = rv ? norms[e.norm_off + row0 + tid] : 0.f;
        sS[tid] = rv ? P[e.scale_off + row0 + tid] : 0.f;
      }
      __syncthreads();
      float v[4][4];
      if (AXIS == 0) dr_tile_ba(sU, sD, r, tx, ty, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + ty * 4 + i;
        float4v h4 = {0.f, 0.f, 0.f, 0.f};
        if (row < e.out && cvalid) {
          const long long at = (long long)row * K + c0 + tx * 4;
          const float4v g4 = dr_ld_bf4(gp + at);
          float4v w4 = {0.f, 0.f, 0.f, 0.f};
          if (AXIS == 0) w4 = dr_ld_bf4(w + at);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float nn = AXIS == 0 ? sN[tx * 4 + k] : sN[ty * 4 + i];
            const float sc = AXIS == 0 ? sS[tx * 4 + k] : sS[ty * 4 + i];
            if (nn != 0.f) {
              h4[k] = (g4[k] * sc) / nn;
              if (AXIS == 0) ds[k] += g4[k] * ((w4[k] + e.s * v[i][k]) / nn);
            }
          }
        }
        *reinterpret_cast<float4v*>(&sH[ty * 4 + i][tx * 4]) = h4;
      }
      __syncthreads();
      for (int o4 = 0; o4 < DR_T / 4; ++o4) {
        const float h0 = sH[o4 * 4][col], h1 = sH[o4 * 4 + 1][col], h2 = sH[o4 * 4 + 2][col], h3 = sH[o4 * 4 + 3][col];
#pragma unroll
        for (int jj = 0; jj < DR_RMAX / 4; ++jj) {
          const int j = jg + 4 * jj;
          if (j < r) {
            const float4v u4 = *reinterpret_cast<const float4v*>(&sU[j][o4 * 4]);
            float a = acc[jj];
            a = fmaf(h0, u4.x, a); a = fmaf(h1, u4.y, a); a = fmaf(h2, u4.z, a); a = fmaf(h3, u4.w, a);
            acc[jj] = a;
          }
        }
      }
      __syncthreads();
    }
    if (col < ncols) {
#pragma unroll
      for (int jj = 0; jj < DR_RMAX / 4; ++jj) {
        const int j = jg + 4 * jj;
        if (j < r) dr_put(dP + e.down_off + (long long)j * K + c0 + col, e.s * acc[jj], accumulate);
      }
    }
  }
  if (AXIS == 0) {
    float (*sRed)[DR_T] = reinterpret_cast<float (*)[DR_T]>(&sH[0][0]);   // 16 x 64 floats of the 64 x 68 tile
#pragma unroll
    for (int k = 0; k < 4; ++k) sRed[ty][tx * 4 + k] = ds[k];
    __syncthreads();
    const float tot = dr_line_sum(sRed, tid);
    if (tid < ncols) dr_put(dP + e.scale_off + ci0 + tid, tot, accumulate);
  }
}

// row owner: 64 rows of one entry, every column.  d_up[o][j] = s sum_c H[o][c] down[j][c] (c ascending); AXIS 1 also
// d_scale[o] = sum G (Weff / n)
template <int AXIS>
__global__ void __launch_bounds__(256) dora_project_rows_kernel(const DoraEntry* __restrict__ tab, int e0, int e1,
                                                                int blk_base, const bf16_t* __restrict__ W,
                                                                const float* __restrict__ P, float* __restrict__ dP,
                                                                const float* __restrict__ norms,
                                                                const bf16_t* __restrict__ G, int accumulate) {
  __shared__ __attribute__((aligned(16))) float sU[AXIS == 1 ? DR_RMAX : 1][DR_LD];
  __shared__ __attribute__((aligned(16))) float sD[DR_RMAX][DR_LD];
  __shared__ __attribute__((aligned(16))) float sH[DR_T][DR_LD];   // H tile transposed [col][row]
  __shared__ float sN[DR_T], sS[DR_T];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lrow = tid & 63, jg = tid >> 6;
  const int bid = blockIdx.x + blk_base;
  const DoraEntry e = tab[dr_find<false>(tab, e0, e1, bid)];
  const int lb = bid - e.rblk0;
  const long long K = (long long)e.kk * e.cin;
  const int r = e.rank;
  const int row0 = lb * DR_T;
  const bf16_t* w = W + e.w_off;
  const bf16_t* gp = G + e.wp_off;
  float ds[4] = {0.f, 0.f, 0.f, 0.f};
  float acc[DR_RMAX / 4];
#pragma unroll
  for (int jj = 0; jj < DR_RMAX / 4; ++jj) acc[jj] = 0.f;
  if (AXIS == 1) {
    dr_load_up(sU, P + e.up_off, row0, e.out, r);
    if (tid < DR_T) {
      const bool rv = row0 + tid < e.out;
      sN[tid] = rv ? norms[e.norm_off + row0 + tid] : 0.f;
      sS[tid] = rv ? P[e.scale_off + row0 + tid] : 0.f;
    }
  }
  for (long long c0 = 0; c0 < K; c0 += DR_T) {
    const int ncols = (int)min((long long)DR_T, K - c0);
    const bool cvalid = tx * 4 < ncols;
    dr_load_down(sD, P + e.down_off, K, c0, ncols, r);
    if (AXIS == 0 && tid < DR_T) {
      const int ci = (int)((c0 + tid) % e.cin);
      sN[tid] = tid < ncols ? norms[e.norm_off + ci] : 0.f;
      sS[tid] = tid < ncols ? P[e.scale_off + ci] : 0.f;
    }
    __syncthreads();
    float v[4][4];
    if (AXIS == 1) dr_tile_ba(sU, sD, r, tx, ty, v);
    float h[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + ty * 4 + i;
#pragma unroll
      for (int k = 0; k < 4; ++k) h[i][k] = 0.f;
      if (row < e.out && cvalid) {
        const long long at = (long long)row * K + c0 + tx * 4;
        const float4v g4 = dr_ld_bf4(gp + at);
        float4v w4 = {0.f, 0.f, 0.f, 0.f};
        if (AXIS == 1) w4 = dr_ld_bf4(w + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float nn = AXIS == 0 ? sN[tx * 4 + k] : sN[ty * 4 + i];
          const float sc = AXIS == 0 ? sS[tx * 4 + k] : sS[ty * 4 + i];
          if (nn != 0.f) {
            h[i][k] = (g4[k] * sc) / nn;
            if (AXIS == 1) ds[i] += g4[k] * ((w4[k] + e.s * v[i][k]) / nn);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4v t = {h[0][k], h[1][k], h[2][k], h[3][k]};
      *reinterpret_cast<float4v*>(&sH[tx * 4 + k][ty * 4]) = t;
    }
    __syncthreads();
    for (int c4 = 0; c4 < DR_T / 4; ++c4) {
      const float h0 = sH[c4 * 4][lrow], h1 = sH[c4 * 4 + 1][lrow], h2 = sH[c4 * 4 + 2][lrow], h3 = sH[c4 * 4 + 3][lrow];
#pragma unroll
      for (int jj = 0; jj < DR_RMAX / 4; ++jj) {
        const int j = jg + 4 * jj;
        if (j < r) {
          const float4v d4 = *reinterpret_cast<const float4v*>(&sD[j][c4 * 4]);
          float a = acc[jj];
          a = fmaf(h0, d4.x, a); a = fmaf(h1, d4.y, a); a = fmaf(h2, d4.z, a); a = fmaf(h3, d4.w, a);
          acc[jj] = a;
        }
      }
    }
    __syncthreads();
  }
  if (row0 + lrow < e.out) {
#pragma unroll
    for (int jj = 0; jj < DR_RMAX / 4; ++jj) {
      const int j = jg + 4 * jj;
      if (j < r) dr_put(dP + e.up_off + (long long)(row0 + lrow) * r + j, e.s * acc[jj], accumulate);
    }
  }
  if (AXIS == 1) {
    float (*sRed)[DR_T] = reinterpret_cast<float (*)[DR_T]>(&sH[0][0]);
#pragma unroll
    for (int i = 0; i < 4; ++i) sRed[tx][ty * 4 + i] = ds[i];
    __syncthreads();
    const float tot = dr_line_sum(sRed, tid);
    if (row0 + tid < e.out && tid < DR_T) dr_put(dP + e.scale_off + row0 + tid, tot, accumulate);
  }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------
OTAMD_API int otamd_dora_entry_size(void) { return (int)sizeof(DoraEntry); }
OTAMD_API int otamd_dora_max_rank(void) { return DR_RMAX; }

// every range entries [e0, e1) name lies inside the buffers, and their workgroup numbering is consecutive: the
// kernels trust the table
static int dora_check(const DoraEntry* t, int e0, int e1, int axis, long long base_numel, long long params_numel,
                      long long norms_numel, long long wp_numel) {
  for (int i = e0; i < e1; ++i) {
    const DoraEntry& e = t[i];
    if (e.out <= 0 || e.cin <= 0 || (e.cin & 3) || e.kk <= 0 || e.kk > 64) return OTAMD_EINVAL;
    if (e.rank <= 0) return OTAMD_EINVAL;
    if (e.rank > DR_RMAX) return OTAMD_EUNSUPPORTED;
    const long long K = (long long)e.kk * e.cin, kept = axis ? e.out : e.cin;
    if (e.w_off < 0 || (e.w_off & 3) || e.w_off + e.out * K > base_numel) return OTAMD_EINVAL;
    if (e.wp_off < 0 || (e.wp_off & 3) || e.wp_off + e.out * K > wp_numel) return OTAMD_EINVAL;
    if (e.down_off < 0 || e.down_off + e.rank * K > params_numel) return OTAMD_EINVAL;
    if (e.up_off < 0 || e.up_off + (long long)e.out * e.rank > params_numel) return OTAMD_EINVAL;
    if (e.scale_off < 0 || e.scale_off + kept > params_numel) return OTAMD_EINVAL;
    if (e.norm_off < 0 || e.norm_off + kept > norms_numel) return OTAMD_EINVAL;
    if (i == e0) continue;
    const DoraEntry& p = t[i - 1];
    if (e.cblk0 != p.cblk0 + ceil_div(p.cin, DR_T) || e.rblk0 != p.rblk0 + ceil_div(p.out, DR_T)) return OTAMD_EINVAL;
  }
  return OTAMD_OK;
}

// table_dev / table_host: the same DoraEntry[n] on the device and on the host (checked here on every call).
// base: bf16 base store; params: fp32 adapter store; norms: fp32 out; wp: bf16 W' out.  axis 0 keeps the input
// channels, 1 the output channels.
OTAMD_API int otamd_dora_merge(const void* table_dev, const void* table_host, int n, int axis, float eps,
                               const void* base, long long base_numel, const float* params, long long params_numel,
                               float* norms, long long norms_numel, void* wp, long long wp_numel, hipStream_t stream) {
  if (!table_dev || !table_host || n < 0 || (axis != 0 && axis != 1) || !base || !params || !norms || !wp)
    return OTAMD_EINVAL;
  if (((uintptr_t)base | (uintptr_t)wp) & 7) return OTAMD_EINVAL;
  if (n == 0) return OTAMD_OK;
  const DoraEntry* t = (const DoraEntry*)table_host;
  if (t[0].cblk0 != 0 || t[0].rblk0 != 0) return OTAMD_EINVAL;
  if (const int rc = dora_check(t, 0, n, axis, base_numel, params_numel, norms_numel, wp_numel)) return rc;
  const DoraEntry& l = t[n - 1];
  const int blocks = axis == 0 ? l.cblk0 + ceil_div(l.cin, DR_T) : l.rblk0 + ceil_div(l.out, DR_T);
  if (axis == 0)
    dora_merge_kernel<0><<<blocks, 256, 0, stream>>>((const DoraEntry*)table_dev, n, (const bf16_t*)base, params, norms,
                                                     (bf16_t*)wp, eps);
  else
    dora_merge_kernel<1><<<blocks, 256, 0, stream>>>((const DoraEntry*)table_dev, n, (const bf16_t*)base, params, norms,
                                                     (bf16_t*)wp, eps);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// entries [e0, e1): G (bf16, the layout of W') -> grads (fp32, the layout of params): overwrite, or add when
// `accumulate`
OTAMD_API int otamd_dora_project(const void* table_dev, const void* table_host, int n, int e0, int e1, int axis,
                                 const void* base, long long base_numel, const float* params, float* grads,
                                 long long params_numel, const float* norms, long long norms_numel, const void* g,
                                 long long g_numel, int accumulate, hipStream_t stream) {
  if (!table_dev || !table_host || e0 < 0 || e1 > n || e0 > e1 || (axis != 0 && axis != 1) || !base || !params ||
      !grads || !norms || !g)
    return OTAMD_EINVAL;
  if (((uintptr_t)base | (uintptr_t)g) & 7) return OTAMD_EINVAL;
  if (e0 == e1) return OTAMD_OK;
  const DoraEntry* t = (const DoraEntry*)table_host;
  if (const int rc = dora_check(t, e0, e1, axis, base_numel, params_numel, norms_numel, g_numel)) return rc;
  const DoraEntry& f = t[e0];
  const DoraEntry& l = t[e1 - 1];
  const int cblocks = l.cblk0 + ceil_div(l.cin, DR_T) - f.cblk0, rblocks = l.rblk0 + ceil_div(l.out, DR_T) - f.rblk0;
  const DoraEntry* td = (const DoraEntry*)table_dev;
  const bf16_t* W = (const bf16_t*)base;
  const bf16_t* G = (const bf16_t*)g;
  if (axis == 0) {
    dora_project_cols_kernel<0><<<cblocks, 256, 0, stream>>>(td, e0, e1, f.cblk0, W, params, grads, norms, G, accumulate);
    dora_project_rows_kernel<0><<<rblocks, 256, 0, stream>>>(td, e0, e1, f.rblk0, W, params, grads, norms, G, accumulate);
  } else {
    dora_project_cols_kernel<1><<<cblocks, 256, 0, stream>>>(td, e0, e1, f.cblk0, W, params, grads, norms, G, accumulate);
    dora_project_rows_kernel<1><<<rblocks, 256, 0, stream>>>(td, e0, e1, f.rblk0, W, params, grads, norms, G, accumulate);
  }
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
