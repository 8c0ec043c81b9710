// Flash attention forward for the AutoencoderKL mid block's single 512-wide head on gfx950 (every VAE this project
// loads: SD 1.5, SDXL, FLUX).  Forward only -- the VAE is frozen -- and no LSE output.  Q [B, Nq, H, 512], K / V
// [B, Nk, H, 512] read in place through the token / batch strides of AttnArgs (the VAE passes column slices of its
// fused [B, N, 3 C] projection), O written with 8-byte vector stores.  Reached from otamd_attn_xwide_fwd.
//
// Why a design of its own.  At D = 512 one 32-query block of O^T is 512 x 32 fp32 = 256 VGPRs per wave and its Q
// fragments another 128: attention_wide.hip's "four waves split the keys of one 32-query block" would need four
// private K / V streams of 2 x 32 KiB each (256 KiB of LDS), and attention.hip's 128-wide O tile does not exist.
// What D = 512 gives in return is 1024 MACs per score: the softmax (16 exp2 per lane and tile) is ~5 % of a tile's
// MFMA time, so nothing needs to overlap it and one wave per SIMD is enough.
//
// Split: rows.  A workgroup owns QT = 128 queries of one (batch, head); wave w owns queries 32 w .. 32 w + 31 with
// all 512 output columns, its Q fragments (B operand of S^T = K Q^T) held in registers for the whole kernel.  No
// P tile and no row statistics cross waves; the only shared data are the K / V tiles.  The column split was the
// alternative: each wave would read only its 128 columns of V (a quarter of the LDS reads in P V), but S needs
// the full 512-deep dot product per score, so either every wave reads all of K anyway and P plus the rescale
// factors go through LDS with two more barriers per tile, or the waves exchange fp32 partial scores (80 bytes
// of LDS per score against 0.5 MFMA cycles per score: 160 B/clk, worse than what it saves).
//   Arithmetic intensity against L2: a tile of KT keys is 2 x KT x 1 KiB of K and V for 4 QT KT 512 flops, i.e. QT
//   flops per byte: 128 with QT = 128 (32 B/clk per CU at the full MFMA rate; QT = 64 would ask 64 B/clk per CU,
//   the whole L2 bandwidth of an XCD).  The price is fill: ceil(Nq / 128) B H workgroups on 256 CUs -- 128 for one
//   1024^2 image (N = 16384), 512 for an encode batch of 4, 32 per 512^2 image.  Small N belongs to the materialized
//   path (kernels.VAE_FLASH_MIN_TOKENS).
//
// MFMA: v_mfma_f32_32x32x16_bf16 (8 passes, 32 cycles), both GEMMs in the transposed form of attention_wide.hip:
// S^T [32 keys x 32 queries] = K Q^T (32 k-steps), O^T [512 x 32 queries] += V^T P^T (16 column tiles x 2 k-steps).
// The query sits on the lane, so the running max / sum are per lane (plus one permlane32 swap between the two lane
// halves), and exp2(S^T) packs straight into the B operand of the second GEMM: P never touches LDS.
//
// LDS (128 KiB, dynamic: needs the opt-in attribute): K ring of two [32 x 512] bf16 images (32 KiB each) and a V
// ring of two.  Tile j + 1 is staged by LDS-DMA (buffer_load_dwordx4 ... lds, 1 KiB = one key row per wave
// instruction, each wave 8 rows of K and 8 of V) right after the barrier that opens tile j, so it has a whole tile of
// MFMAs (64 x 32 cycles) to land; one barrier per tile (BARRIER_LDS after vmcnt(0); its rule, the LDS-DMA and the
// MFMA helpers: mfma_prims.h): every wave's pieces of tile j have landed and every wave's reads of tile j - 1, the
// slot the refill goes to, have retired.
// Rows past Nk are zero-filled through an invalid buffer offset (V: 0 x garbage must not reach O) and masked to -inf.
//   Reads: K by rows (ds_read_b128: lane (r, h) <- key r, columns 16 s + 8 h ..), V transposed
//   (ds_read_b64_tr_b16), each 1 KiB per wave per MFMA.  LDS bytes per MFMA: 1024 per 32 cycles and wave, 128 B/clk
//   for the four SIMDs, half of the 256 B/clk the LDS delivers -- this ratio, not HBM, bounds the kernel, and it is
//   the reason for the 32x32x16 shape (16x16x32 with a 16-query wave: 1 KiB per 16 cycles, 256 B/clk, LDS-bound).
//   Layout: 1024-byte rows (64 chunks of 16 bytes) all start at bank 0, so chunk ch of row r is stored at
//   ch ^ f(r), f(r) = (r & 3) << 2 | (r >> 2) & 3 (the low four chunk bits move, 64 chunks stay 64).  f is a
//   bijection of r mod 16: the sixteen rows of a 16-lane group of the row read land in sixteen different chunk slots
//   (all 64 banks once); r & 3 in chunk bits 2..3 puts the four rows 4 h + q of a transposed read (4 rows x 64 bytes
//   per 32-lane half) into the four 16-bank quarters.  Both reads are conflict-free.
//
// Registers (per wave, one wave per SIMD, 512-entry file): O^T 256 + Q 128 + S^T 16 + P^T 8 + operand fragments and
// addresses; as compiled: see DESIGN.md, "Flash attention for the VAE's 512-wide head".
//
// Softmax: fp32, log2 domain with the scale folded in (exp2(s c - m), c = scale log2 e), lazy running max as in
// attention.hip (m moves only when a score exceeds it by more than 8, so P <= 2^8 before its bf16 rounding), O
// normalised once at the end.  No atomics, fixed order: two runs give the same bits.
//
// Known costs, not yet removed: O leaves the registers as 8-byte stores scattered over 32 rows (64 per lane; 1 / KT
// of a tile's traffic per key tile, once); Q arrives as 32 row-strided 16-byte loads per lane; a wave whose 32
// queries lie past Nq (Nq % 128 <= 96) still runs its MFMAs.
#include "common.h"
#include "attention_args.h"
#include "mfma_prims.h"

#include <cmath>

namespace {

constexpr int DH = 512;               // head width (the only one instantiated)
constexpr int QT = 128;               // queries per workgroup (4 waves x 32)
constexpr int KT = 32;                // keys per tile
constexpr int RB = DH * 2;            // row bytes = one DMA piece
constexpr int IMG = KT * RB;          // one [32 x 512] bf16 image (32 KiB)
constexpr int XW_LDS = 4 * IMG;       // K ring of two, V ring of two
static_assert(RB == 1024, "one key row = one 1 KiB LDS-DMA piece (64 lanes x 16 bytes)");

// chunk swizzle of row r (low four chunk bits)
__device__ __forceinline__ int swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// lane-constant byte offsets into one [32 x 512] image
struct XImg {
  int rowo;     // row read: row r, chunk h (k-step 0); k-step s: ^ (s & 7) << 5, + 256 (s >> 3)
  int tro[2];   // transposed read: rows 4 h + q (+ 8), column tile 0; tile dt: ^ (dt & 3) << 6, + 256 (dt >> 2)
  __device__ __forceinline__ void prepare() {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int G = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    rowo = r * RB + ((h ^ swz(r)) << 4);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int rr = 4 * h + q + 8 * e;
      tro[e] = rr * RB + (((2 * (G & 1) + (p >> 1)) ^ swz(rr)) << 4) + ((p & 1) << 3);
    }
  }
  // row operand, k-step s: lane (r, h) <- row r, elements 16 s + 8 h .. + 7
  __device__ __forceinline__ bf16x8 rowf(const char* img, int s) const {
    return *reinterpret_cast<const bf16x8*>(img + ((rowo ^ ((s & 7) << 5)) + 256 * (s >> 3)));
  }
  // transposed A operand with the accumulator's k order: element j of lane half h <- row 16 s + 8 (j >> 2) + 4 h +
  // (j & 3), column 32 dt + (lane & 31)
  __device__ __forceinline__ bf16x8 trf(const char* img, int s, int dt) const {
    const char* base = img + 16 * RB * s + 256 * (dt >> 2);
    const int x = (dt & 3) << 6;
    return tr16_pair(base, tro[0] ^ x, tro[1] ^ x);
  }
};

// workgroup = 128 queries of one (batch, head); wave w: queries 32 w .. + 31, all keys, all 512 columns
__global__ void __launch_bounds__(256, 1) attn_xwide_fwd_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hh = blockIdx.y, b = blockIdx.z;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * QT + wave * 32;
  const auto rk = rsrc(a.k + b * a.bsk + hh * DH, ((long long)(a.Nk - 1) * a.ldk + DH) * 2);
  const auto rv = rsrc(a.v + b * a.bsv + hh * DH, ((long long)(a.Nk - 1) * a.ldv + DH) * 2);
  const int nt = (a.Nk + KT - 1) / KT;
  XImg im;
  im.prepare();

  // tile j -> ring slot: this wave moves rows 8 w .. 8 w + 7 of K and of V; lane l fills chunk slot l of the row
  // (the row offset is wave-uniform and rides in the scalar offset; the lane's column is recomputed per tile from
  // an opaque copy of the lane id, so no per-row offset registers stay live across the MFMAs)
  auto stage = [&](int j, int slot) {
    int lane16 = lane << 4;
    asm volatile("" : "+v"(lane16));
#pragma unroll
    for (int i = 0; i < KT / 4; ++i) {
      const int p = wave * (KT / 4) + i, key = j * KT + p;
      const bool ok = key < a.Nk;
      const unsigned col = ok ? (unsigned)(lane16 ^ (swz(p) << 4)) : OFF_INVALID;
      dma16(rk, smem + slot * IMG + p * RB, col, ok ? (unsigned)key * (unsigned)a.ldk * 2u : 0u);
      dma16(rv, smem + (2 + slot) * IMG + p * RB, col, ok ? (unsigned)key * (unsigned)a.ldv * 2u : 0u);
    }
  };

  // Q fragments (B operand of S^T): lane (r, h) <- Q[q0 + r][16 s + 8 h .. + 7], zero past Nq
  bf16x8 qf[DH / 16];
  {
    const bool rok = q0 + r < a.Nq;
    const bf16_t* qp = a.q + b * a.bsq + hh * DH + (long long)(rok ? q0 + r : 0) * a.ldq + 8 * h;
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) {
      uint4 t = *reinterpret_cast<const uint4*>(qp + 16 * s);   // a row past Nq reads row 0
      t.x = rok ? t.x : 0u;
      t.y = rok ? t.y : 0u;
      t.z = rok ? t.z : 0u;
      t.w = rok ? t.w : 0u;
      qf[s] = __builtin_bit_cast(bf16x8, t);
    }
  }
  stage(0, 0);

  const float c = a.scale * LOG2E;
  float16v O[DH / 32];
#pragma unroll
  for (int t = 0; t < DH / 32; ++t) O[t] = zero16();
  float m = -INFINITY, l = 0.f;

  for (int j = 0; j < nt; ++j) {
    const int slot = j & 1;
    WAIT_VM();       // this wave's pieces of tile j
    BARRIER_LDS();   // every wave's pieces of tile j; every wave's reads of tile j - 1 (the other slot)
    if (j + 1 < nt) stage(j + 1, slot ^ 1);
    const char* kimg = smem + slot * IMG;
    const char* vimg = smem + (2 + slot) * IMG;

    float16v S = zero16();
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) S = mfma32(im.rowf(kimg, s), qf[s], S);
    if (j * KT + KT > a.Nk) {   // the partial last tile
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j * KT + acc_row(i, h) >= a.Nk) S[i] = -INFINITY;
    }
    float tmax = S[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) tmax = fmaxf(tmax, S[i]);
    // lazy max: m moves only when a score exceeds it by more than RESCALE_T; both lane halves of a query then take
    // the full row's max, so m is the same in both.  Key j KT of a tile is always valid: the new max is finite.
    if (__builtin_amdgcn_ballot_w64(tmax * c > m + RESCALE_T) != 0) {
      const float mn = fmaxf(m, fmaxf(tmax, xor32(tmax)) * c);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < DH / 32; ++dt)
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
    {
      bf16x8 v0 = im.trf(vimg, 0, 0), v1 = im.trf(vimg, 1, 0);
#pragma unroll
      for (int dt = 0; dt < DH / 32; ++dt) {
        const bf16x8 c0 = v0, c1 = v1;
        if (dt + 1 < DH / 32) {
          v0 = im.trf(vimg, 0, dt + 1);
          v1 = im.trf(vimg, 1, dt + 1);
        }
        O[dt] = mfma32(c0, p0, O[dt]);
        O[dt] = mfma32(c1, p1, O[dt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // O[q][32 dt + 8 g + 4 h + e] = O^T register 4 g + e of tile dt: four columns = one 8-byte store
  // (lane id and row pointer are formed afresh here: neither may occupy registers during the loop)
  int le;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(le));
  {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
    l += __uint_as_float((le & 32) ? s[0] : s[1]);
  }
  const int qe = q0 + (le & 31);
  if (qe < a.Nq) {
    const float inv = 1.f / l;
    bf16_t* op = a.o + b * a.bso + hh * DH + (long long)qe * a.ldo + 4 * (le >> 5);
#pragma unroll
    for (int dt = 0; dt < DH / 32; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 pk;
        pk.x = (uint32_t)f2bf(O[dt][4 * g] * inv) | ((uint32_t)f2bf(O[dt][4 * g + 1] * inv) << 16);
        pk.y = (uint32_t)f2bf(O[dt][4 * g + 2] * inv) | ((uint32_t)f2bf(O[dt][4 * g + 3] * inv) << 16);
        *reinterpret_cast<uint2*>(op + 32 * dt + 8 * g) = pk;
      }
  }
}

}   // namespace

OTAMD_API int otamd_attn_xwide_fwd(const AttnArgs* in, hipStream_t stream) {
  if (!in || !in->q || !in->k || !in->v || !in->o) return OTAMD_EINVAL;
  const AttnArgs& a = *in;
  if (a.B <= 0 || a.H <= 0 || a.Nq <= 0 || a.Nk <= 0 || a.Dv != DH) return OTAMD_EINVAL;
  if (a.B > 65535 || a.H > 65535) return OTAMD_EINVAL;   // grid y / z
  if (!(a.scale > 0.f) || !std::isfinite(a.scale)) return OTAMD_EINVAL;   // masked keys are -inf after the scale
  const long long lds[] = {a.ldq, a.ldk, a.ldv, a.ldo, a.bsq, a.bsk, a.bsv, a.bso};
  for (long long v : lds)
    if (v % 8) return OTAMD_EINVAL;   // 16-byte row loads, 8-byte row stores
  if (a.ldq < (long long)a.H * DH || a.ldk < (long long)a.H * DH || a.ldv < (long long)a.H * DH ||
      a.ldo < (long long)a.H * DH)
    return OTAMD_EINVAL;
  if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.o) & 15) return OTAMD_EINVAL;
  if (!fits31(a.Nk, a.ldk, DH) || !fits31(a.Nk, a.ldv, DH)) return OTAMD_EINVAL;
  attn_launch(attn_xwide_fwd_kernel, dim3((a.Nq + QT - 1) / QT, a.H, a.B), XW_LDS, stream, a);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}
