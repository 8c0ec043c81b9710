// Flash attention forward / backward for 160-wide heads on gfx950 (SD 1.5's 1280-channel levels: 8 heads of 160;
// any head dim 128 < Dv <= 160, Dv % 8 == 0, zero-filled to DW = 160).  Same interface as attention.hip: Q [B, Nq, H, D],
// K / V [B, Nk, H, D] read in place through the token / batch strides of AttnArgs, LSE per (b, h, q) in the log2
// domain; reached from otamd_attn_fwd / otamd_attn_bwd(_ex) for Dv > 128.
//
// Why a design of its own.  The SD 1.5 deep levels are small: 256 tokens (down 2 / up 1) or 64 (mid) at 512^2, 8
// heads, 77 text keys.  128-query workgroups (attention.hip) would give 64 workgroups on 256 CUs, and a 160-wide
// O^T accumulator (80 VGPRs) beside 40 VGPRs of Q fragments leaves no room for more than one wave per SIMD anyway.
// So the split is the other way round: a workgroup owns ONE 32-row block (32 queries in forward / dQ, 32 keys in
// dK/dV) and its four waves split the streamed dimension between them -- wave w takes the 32-row sub-tiles w, w+4,
// w+8, ... of the keys (forward, dQ) or of the queries (dK/dV).  Each wave runs a complete flash loop over its
// sub-tiles (own running max / sum, own accumulators); at the end the four partial results meet once in LDS and are
// combined in wave order 0, 1, 2, 3 (log-sum-exp weights in the forward, plain sums in the backward).  Fixed order,
// no atomics, no fp32 slabs in HBM, no cast launch: two runs give the same bits.
//   Fill (workgroups / 256 CUs, one workgroup per CU: 512 VGPRs per wave, 100 KiB LDS), B = 4, H = 8:
//     Nq = 256: fwd / dQ 256 (1.0);  Nq = 64: 64 (0.25);  Nq = 576: 576 (2.25);  Nq = 1024: 1024 (4.0)
//     Nk = 256: dK/dV 256 (1.0);  Nk = 64: 64 (0.25);  Nk = 77: 96 (0.375);  Nk = 576 / 1024: 2.25 / 4.0
//   Nk = 77 keeps three of the four waves busy in forward / dQ (one 32-key sub-tile each, the last partial).
//   Measured: ahead of the materialized path wherever B H Nq Nk <= 2.5 M scores (a few rounds of short
//   flash loops against ~15 launches on a partly filled chip), behind it from 8.4 M scores on (16 x 8 x 256 x 256,
//   4 x 8 x 576 x 576 and larger), so the Python layer routes 160-wide heads to these kernels up to 2^22 scores.
//
// Data movement.  No tile is shared between waves, so there is no workgroup barrier in any tile loop: a wave
// synchronises only with its own counters (s_waitcnt vmcnt / lgkmcnt); the refill of a wave's own slot is issued
// after s_waitcnt lgkmcnt(0).  The barriers of the final combine are BARRIER_LDS (its rule and the LDS-DMA's:
// mfma_prims.h, which also holds the MFMA helpers).
//   MFMA row operands (A of S^T = K Q^T, dP^T = V dO^T, S = Q K^T, dP = dO V^T) need no transposition: they are loaded
//   from HBM/L2 straight into registers, 16 bytes per lane, one sub-tile ahead (the registers are the double buffer).
//   Transposed operands (V^T for O^T, K^T for dQ^T, dO^T / Q^T for dV^T / dK^T) go HBM/L2 -> LDS by LDS-DMA into the
//   wave's private 20 KiB region and are read with ds_read_b64_tr_b16.  Forward: V ring of two 10 KiB images.  dQ: K
//   ring of two images, each read twice -- by rows (ds_read_b128) for S^T and transposed for dQ^T.  dK/dV: one slot of
//   a Q and a dO image; its refill lands under the next sub-tile's S / dP MFMAs and softmax.  The block's own K / V
//   rows (the B operands of S / dP) sit in one workgroup-shared pair of images, loaded once before the loop.
//   The 20 KiB region then holds the wave's fp32 partial [160][32] for the combine (dK and dV take turns).
//
// LDS layout (320-byte rows = 20 chunks of 16 bytes, not a power of two): natural 320-byte pitch, chunk ch of row r
// stored at ch ^ ((r >> 2) & 3).  Only the low two chunk bits move, so 20 chunks stay 20.  A row starts at bank
// 16 r mod 64, i.e. rows r .. r+3 cover the four 16-bank quarters: the transposed read (4 rows x 64 bytes per 32-lane
// half) is conflict-free as it stands, and the XOR by r >> 2 separates the rows that share a quarter inside each
// 16-lane group of the b128 row read ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}: r >> 2 = {0, 3, 5, 6} / {1, 2, 4, 7},
// distinct mod 4).  tools/lds_bank_model.py: row reads 40 cycles, transposed reads 40 cycles per 32-row image, both
// the conflict-free cost (unswizzled: 160 / 40).  DMA: a 10 KiB image is 10 wave instructions of 1 KiB; lane l of piece
// p fills bytes [1024 p + 16 l, +16), the swizzle applied on the source address; rows past the operand and columns
// past Dv are zero-filled through an invalid offset.
//
// Registers (per wave): forward O^T 80 + Q 40 + K 40; dQ: dQ^T 80 + Q 40 + dO 40 + V 40 + P^T / dP^T 32; dK/dV: dK^T 80 + dV^T 80 +
// Q rows 40 + dO rows 40 (its K / V fragments are read from a shared LDS image instead of held) -- hence one wave
// per SIMD with the 512-entry file.
//
// Known costs, not yet removed: the four waves of a forward / dQ workgroup each load the block's Q (and dO) fragments;
// every 32-query block re-reads all of K / V from L2 (4x the traffic of 128-query blocks: the backward loses to the
// materialized path at 576 x 576); dQ recomputes S / dP of all but a wave's last sub-tile for its second pass (none
// up to 128 keys); against a one-pass dQ that takes delta = rowsum(dO o O) from the stored O the dQ kernel measures
// (B = 4, H = 8, us, two-pass / one-pass) 7.7 / 9.4 at 64 x 64, 9.0 / 11.2 at 256 x 77, 30.3 / 36.9 at 1024 x 77 (no
// recompute, and no O rows to load), 15.0 / 15.2 at 256 x 256, 62.7 / 46.9 at 576 x 576, 122.9 / 84.0 at 1024 x 1024
// (the last two are routed to the materialized path); the dK/dV kernel fetches its {lse, delta} pairs as 16 scattered 8-byte loads per lane and
// sub-tile and spills 5 VGPRs (24 bytes of scratch per lane) at 256 + 256 registers.
#include "common.h"
#include "attention_args.h"
#include "mfma_prims.h"

namespace {

constexpr int DW = 160;               // padded head width
constexpr int RB = DW * 2;            // row bytes
constexpr int IMG = 32 * RB;          // one [32 x 160] bf16 image (10 KiB)
constexpr int NPIECE = IMG / 1024;    // DMA pieces per image
constexpr int REGION = 2 * IMG;       // a wave's private LDS (20 KiB) = its fp32 partial [160][32]
constexpr int SHARED = 4 * REGION;    // after the four regions: the forward's {m, l} table / dK/dV's K and V images
constexpr int WIDE_LDS = SHARED + 2 * IMG;   // 100 KiB

__device__ __forceinline__ int wsw(int r) { return (r >> 2) & 3; }

// lane-constant geometry of one [32 x 160] image: the DMA source of every piece, the b128 row reads and the
// transposed reads
struct WideImg {
  int src[NPIECE];   // row << 16 | first element column of the chunk this lane moves in piece p
  int rowo[2];       // byte offset of the row read, k-step s even / odd (+ 64 (s >> 1))
  int tro[2];        // byte offset of the transposed read, rows 4h + q (+ 8), column block 0 (+ 64 dt, + 16 RB s)
  __device__ __forceinline__ void prepare() {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int G = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
      const int byte = i * 1024 + lane * 16;
      const int row = byte / RB, pos = (byte % RB) >> 4;
      src[i] = (row << 16) | ((pos ^ wsw(row)) << 3);
    }
    rowo[0] = r * RB + ((h ^ wsw(r)) << 4);
    rowo[1] = r * RB + (((2 | h) ^ wsw(r)) << 4);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int rr = 4 * h + q + 8 * e;
      tro[e] = rr * RB + (((2 * (G & 1) + (p >> 1)) ^ wsw(rr)) << 4) + ((p & 1) << 3);
    }
  }
  // rows [row0, row0 + 32) of a [nrows x ld] operand whose descriptor starts at (batch, head) -> img
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, char* img, long long ld, int row0, int nrows,
                                        int Dv) const {
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
      const int rr = row0 + (src[i] >> 16), col = src[i] & 0xffff;
      const unsigned off = (rr < nrows && col < Dv) ? (unsigned)(rr * (int)ld + col) * 2u : OFF_INVALID;
      dma16(rs, img + i * 1024, off);
    }
  }
  // one piece, chosen at run time (wave-uniform): the workgroup-shared images
  static __device__ __forceinline__ void issue_piece(__amdgpu_buffer_rsrc_t rs, char* img, long long ld, int row0,
                                                     int nrows, int Dv, int piece) {
    const int byte = piece * 1024 + (threadIdx.x & 63) * 16;
    const int row = byte / RB, col = (((byte % RB) >> 4) ^ wsw(row)) << 3;
    const unsigned off = (row0 + row < nrows && col < Dv) ? (unsigned)((row0 + row) * (int)ld + col) * 2u : OFF_INVALID;
    dma16(rs, img + piece * 1024, off);
  }
  // row operand, k-step s: lane (r, h) <- row r, elements 16 s + 8 h .. + 7
  __device__ __forceinline__ bf16x8 rowf(const char* img, int s) const {
    return *reinterpret_cast<const bf16x8*>(img + rowo[s & 1] + 64 * (s >> 1));
  }
  // transposed A operand with the accumulator's k order: element j of lane half h <- row 16 s + 8 (j >> 2) + 4 h +
  // (j & 3), column 32 dt + (lane & 31)
  __device__ __forceinline__ bf16x8 trf(const char* img, int s, int dt) const {
    const char* base = img + 16 * RB * s + 64 * dt;
    return tr16_pair(base, tro[0], tro[1]);
  }
};

// row fragments straight from memory: lane (r, h) <- X[row0 + r][16 s + 8 h .. + 7], zero past nrows / Dv
__device__ __forceinline__ void load_rows(bf16x8 (&f)[DW / 16], const bf16_t* base, long long ld, int row0, int nrows,
                                          int Dv) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const bool rok = row0 + r < nrows;
  const bf16_t* p = base + (long long)(rok ? row0 + r : 0) * ld;
#pragma unroll
  for (int s = 0; s < DW / 16; ++s) {
    const int d = 16 * s + 8 * h;
    if (rok && d < Dv) f[s] = *reinterpret_cast<const bf16x8*>(p + d);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[s][j] = (__bf16)0.f;
    }
  }
}

// this wave's accumulators (row = head column acc_row, lane = the block's row r) -> its fp32 partial [160][32]
__device__ __forceinline__ void put_partial(char* region, const float16v (&X)[DW / 32]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  float* part = reinterpret_cast<float*>(region);
#pragma unroll
  for (int dt = 0; dt < DW / 32; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) part[(dt * 32 + acc_row(i, h)) * 32 + r] = X[dt][i];
}

// out[row0 + row][d] = mul * sum_w wgt[w] * partial_w[d][row], waves in order 0..3; thread t <-> row t & 31, head
// columns 20 (t >> 5) .. + 19 (five 8-byte stores)
__device__ __forceinline__ void combine(const char* smem, const float (&wgt)[4], float mul, bf16_t* out, long long ld,
                                        int row0, int nrows, int Dv) {
  const int row = threadIdx.x & 31, dg = threadIdx.x >> 5;
  if (row0 + row >= nrows) return;
  bf16_t* op = out + (long long)(row0 + row) * ld;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const int d0 = dg * 20 + 4 * c;
    if (d0 >= Dv) break;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        acc = fmaf(wgt[w], reinterpret_cast<const float*>(smem + w * REGION)[(d0 + e) * 32 + row], acc);
      v[e] = acc * mul;
    }
    uint2 pk;
    pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *reinterpret_cast<uint2*>(op + d0) = pk;
  }
}

// ------------------------------------------------------------------------------------------
// forward: workgroup = 32 queries of one (batch, head); wave w: key sub-tiles w, w + 4, ...
__global__ void __launch_bounds__(256, 1) attn_wide_fwd_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hh = blockIdx.y, b = blockIdx.z;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const bf16_t* Kp = a.k + b * a.bsk + hh * a.Dv;
  const auto rv = rsrc(a.v + b * a.bsv + hh * a.Dv, ((long long)(a.Nk - 1) * a.ldv + a.Dv) * 2);
  WideImg im;
  im.prepare();
  char* ring = smem + wave * REGION;
  const int nt = (a.Nk + 31) / 32;

  bf16x8 qf[DW / 16], kf[DW / 16];
  load_rows(qf, a.q + b * a.bsq + hh * a.Dv, a.ldq, q0, a.Nq, a.Dv);
  if (wave < nt) {
    im.issue(rv, ring, a.ldv, wave * 32, a.Nk, a.Dv);
    load_rows(kf, Kp, a.ldk, wave * 32, a.Nk, a.Dv);
  }
  const float c = a.scale * LOG2E;
  float16v O[DW / 32];
#pragma unroll
  for (int t = 0; t < DW / 32; ++t) O[t] = zero16();
  float m = -INFINITY, l = 0.f;

  int slot = 0;
  for (int j = wave; j < nt; j += 4, slot ^= 1) {
    WAIT_VM();   // this sub-tile's V image (and K fragments)
    float16v S = zero16();
#pragma unroll
    for (int s = 0; s < DW / 16; ++s) S = mfma32(kf[s], qf[s], S);
    if (j + 4 < nt) {   // the other slot's reads (previous sub-tile) have retired before its refill
      WAIT_LDS();
      im.issue(rv, ring + (slot ^ 1) * IMG, a.ldv, (j + 4) * 32, a.Nk, a.Dv);
      load_rows(kf, Kp, a.ldk, (j + 4) * 32, a.Nk, a.Dv);
    }
    if (j * 32 + 32 > a.Nk) {   // the partial last sub-tile
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j * 32 + acc_row(i, h) >= a.Nk) S[i] = -INFINITY;
    }
    float tmax = S[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) tmax = fmaxf(tmax, S[i]);
    // lazy max as in attention.hip: m moves only when a score exceeds it by more than RESCALE_T; both lane halves
    // of a query then take the full row's max, so m is the same in both
    if (__builtin_amdgcn_ballot_w64(tmax * c > m + RESCALE_T) != 0) {
      const float mn = fmaxf(m, fmaxf(tmax, xor32(tmax)) * c);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < DW / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) O[dt][i] *= alpha;
      m = mn;
    }
    float r0 = 0.f, r1 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      S[i] = __builtin_amdgcn_exp2f(fmaf(S[i], c, -m));
      S[i + 1] = __builtin_amdgcn_exp2f(fmaf(S[i + 1], c, -m));
      r0 += S[i];
      r1 += S[i + 1];
    }
    l += r0 + r1;   // this lane's half-row
    const bf16x8 p0 = pack_acc(S, 0), p1 = pack_acc(S, 1);
    const char* vimg = ring + slot * IMG;
#pragma unroll
    for (int dt = 0; dt < DW / 32; ++dt) {
      O[dt] = mfma32(im.trf(vimg, 0, dt), p0, O[dt]);
      O[dt] = mfma32(im.trf(vimg, 1, dt), p1, O[dt]);
    }
  }
  WAIT_VM();
  l += xor32(l);
  WAIT_LDS();
  put_partial(ring, O);
  float2* ml = reinterpret_cast<float2*>(smem + SHARED);
  if (h == 0) ml[wave * 32 + r] = make_float2(m, l);
  BARRIER_LDS();
  // combine: O = sum_w 2^(m_w - M) O_w / sum_w 2^(m_w - M) l_w; a wave without keys has m = -inf, l = 0 -> weight 0
  const int row = threadIdx.x & 31;
  float mw[4], lw[4], wgt[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float2 t = ml[w * 32 + row];
    mw[w] = t.x;
    lw[w] = t.y;
  }
  const float M = fmaxf(fmaxf(mw[0], mw[1]), fmaxf(mw[2], mw[3]));   // finite: wave 0 always has a key
  float L = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    wgt[w] = __builtin_amdgcn_exp2f(mw[w] - M);
    L = fmaf(wgt[w], lw[w], L);
  }
  combine(smem, wgt, 1.f / L, a.o + b * a.bso + hh * a.Dv, a.ldo, q0, a.Nq, a.Dv);
  if (threadIdx.x < 32 && q0 + row < a.Nq) a.lse[((long long)b * a.H + hh) * a.Nq + q0 + row] = M + __log2f(L);
}

// ------------------------------------------------------------------------------------------
// dQ: the forward's split, in two passes over the wave's key sub-tiles.  delta = sum_j P_j dP_j is formed here in
// fp32 from the very P that enters dS (P rounded to bf16 first, as the dV operand is), not from the stored bf16 O: for a
// one-hot row P = 1 exactly and dS = P (dP - delta) cancels exactly, where rowsum(dO o O) left a 2^-9 |dO . v| residue
// on the peaked key.  Pass 1: S^T, dP^T, P^T per sub-tile -> the wave's partial delta; the four partials meet in LDS
// and are summed in wave order.  Pass 2 walks the sub-tiles backwards: the last one's P^T / dP^T are still in
// registers and its K image in its slot (no recompute up to 128 keys); earlier ones are recomputed bit for bit.
// Publishes {lse, delta} per query for the dK/dV kernel.
__global__ void __launch_bounds__(256, 1) attn_wide_dq_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hh = blockIdx.y, b = blockIdx.z;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const bf16_t* Vp = a.v + b * a.bsv + hh * a.Dv;
  const auto rk = rsrc(a.k + b * a.bsk + hh * a.Dv, ((long long)(a.Nk - 1) * a.ldk + a.Dv) * 2);
  WideImg im;
  im.prepare();
  char* ring = smem + wave * REGION;
  const int nt = (a.Nk + 31) / 32;

  bf16x8 qf[DW / 16], gf[DW / 16], vf[DW / 16];
  load_rows(qf, a.q + b * a.bsq + hh * a.Dv, a.ldq, q0, a.Nq, a.Dv);
  load_rows(gf, a.dout + b * a.bsdo + hh * a.Dv, a.lddo, q0, a.Nq, a.Dv);
  const int q = q0 + r;
  const long long srow = ((long long)b * a.H + hh) * a.Nq;
  const float lse2 = q < a.Nq ? a.lse[srow + q] : 0.f;
  if (wave < nt) {
    im.issue(rk, ring, a.ldk, wave * 32, a.Nk, a.Dv);
    load_rows(vf, Vp, a.ldv, wave * 32, a.Nk, a.Dv);
  }
  const float c = a.scale * LOG2E;
  float16v dQ[DW / 32];
#pragma unroll
  for (int t = 0; t < DW / 32; ++t) dQ[t] = zero16();

  // P^T (bf16 values) and dP^T of key sub-tile j, its K image in kimg and its V rows in vf
  float16v S, dP;
  auto scores = [&](const char* kimg, int j) {
    S = zero16();
    dP = zero16();
#pragma unroll
    for (int s = 0; s < DW / 16; ++s) {
      S = mfma32(im.rowf(kimg, s), qf[s], S);
      dP = mfma32(vf[s], gf[s], dP);
    }
    if (j * 32 + 32 > a.Nk) {   // the partial last sub-tile
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j * 32 + acc_row(i, h) >= a.Nk) S[i] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = (float)(__bf16)__builtin_amdgcn_exp2f(fmaf(S[i], c, -lse2));
  };
  auto prefetch = [&](int j, int slot, bool image) {   // the slot's reads have retired before its refill
    WAIT_LDS();
    if (image) im.issue(rk, ring + slot * IMG, a.ldk, j * 32, a.Nk, a.Dv);
    load_rows(vf, Vp, a.ldv, j * 32, a.Nk, a.Dv);
  };

  float dpart = 0.f;
  int slot = 0, jl = -1, slotl = 0;
  for (int j = wave; j < nt; j += 4, slot ^= 1) {
    WAIT_VM();
    scores(ring + slot * IMG, j);
    if (j + 4 < nt) prefetch(j + 4, slot ^ 1, true);
#pragma unroll
    for (int i = 0; i < 16; ++i) dpart = fmaf(S[i], dP[i], dpart);
    jl = j;
    slotl = slot;
  }
  dpart += xor32(dpart);
  float* dtab = reinterpret_cast<float*>(smem + SHARED);
  if (h == 0) dtab[wave * 32 + r] = dpart;
  BARRIER_LDS();
  const float dlt = ((dtab[r] + dtab[32 + r]) + dtab[64 + r]) + dtab[96 + r];
  if (wave == 0 && h == 0 && q < a.Nq)
    reinterpret_cast<float2*>(const_cast<float*>(a.delta))[srow + q] = make_float2(lse2, dlt);

  slot = slotl;
  for (int j = jl; j >= 0; j -= 4, slot ^= 1) {
    const char* kimg = ring + slot * IMG;
    if (j != jl) {
      WAIT_VM();
      scores(kimg, j);
    }
    if (j - 4 >= 0) prefetch(j - 4, slot ^ 1, j != jl);   // pass 1 left sub-tile jl - 4's image in the other slot
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] *= dP[i] - dlt;   // dS^T
    const bf16x8 s0 = pack_acc(S, 0), s1 = pack_acc(S, 1);
#pragma unroll
    for (int dt = 0; dt < DW / 32; ++dt) {
      dQ[dt] = mfma32(im.trf(kimg, 0, dt), s0, dQ[dt]);
      dQ[dt] = mfma32(im.trf(kimg, 1, dt), s1, dQ[dt]);
    }
  }
  WAIT_VM();
  WAIT_LDS();
  put_partial(ring, dQ);
  BARRIER_LDS();
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  combine(smem, one, a.scale, a.dq + b * a.bsdq + hh * a.Dv, a.lddq, q0, a.Nq, a.Dv);
}

// ------------------------------------------------------------------------------------------
// dK, dV: workgroup = 32 keys of one (batch, head), their K / V images shared in LDS (row reads: as registers they
// would push the wave past the 256 architectural VGPRs beside 160 accumulators); wave w: query sub-tiles w, w + 4, ...
// S = Q K^T and dP = dO V^T with the key on the lane (Q / dO rows from memory), P and dS feed dV^T += dO^T P and
// dK^T += Q^T dS as B operands, dO^T / Q^T by transposed reads of the wave's LDS slot.  One barrier before the loop
// (the shared images), none inside.
__global__ void __launch_bounds__(256, 1) attn_wide_dkv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hh = blockIdx.y, b = blockIdx.z;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int k0 = blockIdx.x * 32;
  const bf16_t* Qp = a.q + b * a.bsq + hh * a.Dv;
  const bf16_t* Gp = a.dout + b * a.bsdo + hh * a.Dv;
  const auto rq = rsrc(Qp, ((long long)(a.Nq - 1) * a.ldq + a.Dv) * 2);
  const auto rg = rsrc(Gp, ((long long)(a.Nq - 1) * a.lddo + a.Dv) * 2);
  const float2* pairs = reinterpret_cast<const float2*>(a.delta) + ((long long)b * a.H + hh) * a.Nq;
  WideImg im;
  im.prepare();
  char* qimg = smem + wave * REGION;
  char* gimg = qimg + IMG;
  const int nt = (a.Nq + 31) / 32;

  bf16x8 qr[DW / 16], gr[DW / 16];
  const char* kimg = smem + SHARED;
  const char* vimg = kimg + IMG;
  {   // 2 x 10 pieces over 4 waves; rows past Nk zero
    const auto rk = rsrc(a.k + b * a.bsk + hh * a.Dv, ((long long)(a.Nk - 1) * a.ldk + a.Dv) * 2);
    const auto rv = rsrc(a.v + b * a.bsv + hh * a.Dv, ((long long)(a.Nk - 1) * a.ldv + a.Dv) * 2);
    for (int t = 0; t < 5; ++t) {
      const int p = wave * 5 + t;
      if (p < NPIECE) WideImg::issue_piece(rk, smem + SHARED, a.ldk, k0, a.Nk, a.Dv, p);
      else WideImg::issue_piece(rv, smem + SHARED + IMG, a.ldv, k0, a.Nk, a.Dv, p - NPIECE);
    }
  }
  if (wave < nt) {
    im.issue(rq, qimg, a.ldq, wave * 32, a.Nq, a.Dv);
    im.issue(rg, gimg, a.lddo, wave * 32, a.Nq, a.Dv);
    load_rows(qr, Qp, a.ldq, wave * 32, a.Nq, a.Dv);
    load_rows(gr, Gp, a.lddo, wave * 32, a.Nq, a.Dv);
  }
  const float c = a.scale * LOG2E;
  float16v dK[DW / 32], dV[DW / 32];
#pragma unroll
  for (int t = 0; t < DW / 32; ++t) { dK[t] = zero16(); dV[t] = zero16(); }
  WAIT_VM();
  BARRIER_LDS();   // the shared K / V images

  for (int j = wave; j < nt; j += 4) {
    // {lse, delta} of the queries this lane's registers hold (acc_row); a query past Nq gets lse = +inf: P = 0
    float ls[16], de[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qi = j * 32 + acc_row(i, h);
      const float2 t = qi < a.Nq ? pairs[qi] : make_float2(INFINITY, 0.f);
      ls[i] = t.x;
      de[i] = t.y;
    }
    float16v S = zero16(), dP = zero16();
#pragma unroll
    for (int s = 0; s < DW / 16; ++s) {
      S = mfma32(qr[s], im.rowf(kimg, s), S);
      dP = mfma32(gr[s], im.rowf(vimg, s), dP);
    }
    // a key past Nk (zero K / V fragments) gets a finite P <= 2^(-lse + |..|) of its own lane only; never stored
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = (float)(__bf16)__builtin_amdgcn_exp2f(fmaf(S[i], c, -ls[i]));   // the dQ kernel's P
      dP[i] = p * (dP[i] - de[i]);
      S[i] = p;
    }
    const bf16x8 p0 = pack_acc(S, 0), p1 = pack_acc(S, 1), d0 = pack_acc(dP, 0), d1 = pack_acc(dP, 1);
    WAIT_VM();   // this sub-tile's Q / dO images
    if (j + 4 < nt) {
      load_rows(qr, Qp, a.ldq, (j + 4) * 32, a.Nq, a.Dv);
      load_rows(gr, Gp, a.lddo, (j + 4) * 32, a.Nq, a.Dv);
    }
#pragma unroll
    for (int dt = 0; dt < DW / 32; ++dt) {
      dV[dt] = mfma32(im.trf(gimg, 0, dt), p0, dV[dt]);
      dV[dt] = mfma32(im.trf(gimg, 1, dt), p1, dV[dt]);
      dK[dt] = mfma32(im.trf(qimg, 0, dt), d0, dK[dt]);
      dK[dt] = mfma32(im.trf(qimg, 1, dt), d1, dK[dt]);
    }
    if (j + 4 < nt) {
      WAIT_LDS();   // the slot's reads have retired before its refill
      im.issue(rq, qimg, a.ldq, (j + 4) * 32, a.Nq, a.Dv);
      im.issue(rg, gimg, a.lddo, (j + 4) * 32, a.Nq, a.Dv);
    }
  }
  WAIT_VM();
  WAIT_LDS();
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  put_partial(qimg, dK);
  BARRIER_LDS();
  combine(smem, one, a.scale, a.dk + b * a.bsdk + hh * a.Dv, a.lddk, k0, a.Nk, a.Dv);
  BARRIER_LDS();   // every wave's reads of the dK partials have retired
  put_partial(qimg, dV);
  BARRIER_LDS();
  combine(smem, one, 1.f, a.dv + b * a.bsdv + hh * a.Dv, a.lddv, k0, a.Nk, a.Dv);
}

}   // namespace

// Called by otamd_attn_fwd / otamd_attn_bwd (attention.hip) with checked arguments, 128 < Dv <= 160.
int otamd_attn_wide_fwd(const AttnArgs& a, hipStream_t stream) {
  attn_launch(attn_wide_fwd_kernel, dim3((a.Nq + 31) / 32, a.H, a.B), WIDE_LDS, stream, a);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

// workspace: one {lse, delta} pair per query (written by the dQ kernel, read by dK/dV); no partial slabs
long long otamd_attn_wide_ws_bytes(const AttnArgs& a) { return (long long)a.B * a.H * a.Nq * 8 + 256; }

int otamd_attn_wide_bwd(const AttnArgs& in, float* ws, hipStream_t stream) {
  AttnArgs a = in;
  a.delta = ws;
  attn_launch(attn_wide_dq_kernel, dim3((a.Nq + 31) / 32, a.H, a.B), WIDE_LDS, stream, a);
  attn_launch(attn_wide_dkv_kernel, dim3((a.Nk + 31) / 32, a.H, a.B), WIDE_LDS, stream, a);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
