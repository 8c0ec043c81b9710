// Operand-tile index decode of the v2 GEMM engine (gemm2_kernel.h): which source element each lane of each
// 1 KiB DMA piece fetches for the K tile at k0, for every operand mode.  Plain integer code, __host__ __device__, with
// no HIP types: tests/csrc/conv_index_check.cpp walks it on the CPU for every lane and piece.
//
// Two forms of the conv gathers:
//   offsets()       closed form: the (tap, channel) / (image, row, column) decode of k by integer division, from
//                   scratch at any k0.  The reference; also what a split's first K tile starts from (start()).
//   offsets_step()  incremental form: k advances by exactly 64 per K-step, so every decoded quantity is carried as a
//                   mixed-radix counter (add the digits of 64, carry at most once per digit: adds and compares only),
//                   and what does not depend on k is decoded once in prepare().  Returns the offsets of the current
//                   K tile and moves the state to the next.  Same offsets as offsets(), no division.
#pragma once

#if defined(__HIPCC__)
#define OTAMD_HD __host__ __device__ __forceinline__
#else
#define OTAMD_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define OTAMD_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)   // launch-uniform value: keep it in a scalar register
#else
#define OTAMD_UNIFORM(x) (x)
#endif

// OPM_CONV_WT (v2 only): B of conv dgrad read straight from the stored weight W[Cout][KH][KW][Cin] as
// an MN-mode operand B[k = tap*Cout + co][ci] (row address (co*KK + tap)*ld); gb.SC = Cout, gb.KH/KW.
enum { OPM_K = 0, OPM_MN = 1, OPM_CONV_FWD = 2, OPM_CONV_DGRAD = 3, OPM_CONV_WGRAD = 4, OPM_CONV_WT = 5 };

struct ConvGeom {
  int N;             // batch
  int SH, SW, SC;    // gathered (source) tensor: spatial dims and channel count
  int RH, RW;        // spatial dims decoding a GEMM row index (fwd: output, dgrad: input, wgrad: output)
  int KH, KW, stride, pad;
  int upsample;      // source read through a virtual nearest-2x upsample (fwd / wgrad)
  int pad_;
  long long ld;      // pixel stride of the source, elements
};

#define OFF_INVALID 0x80000000u

// MN-mode LDS image: [64 k rows][RB bytes], 32-byte block b of row k stored at b ^ s(k)
OTAMD_HD int mn_swz(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }
// the same for an image of RB-byte rows: a 64-wide tile (128-byte rows) has only 4 blocks per row
// and 160-wide tiles (320-byte rows, 10 blocks): the 80-dword row pitch already spreads rows k..k+3 over
// four 8-bank groups; rows k+8.. alias them, so block bit 0 flips with k bit 3 (stays inside the row)
template <int RB> OTAMD_HD int mn_swz_rb(int k) {
  return RB == 320 ? ((k >> 3) & 1) : (RB >= 256 ? mn_swz(k) : (k & 3));
}

template <int MODE> struct IsKMode {
  static constexpr bool v = (MODE == OPM_K || MODE == OPM_CONV_FWD || MODE == OPM_CONV_DGRAD);
};

// v = (hi * r1 + mid) * r0 + lo with 0 <= lo < r0, 0 <= mid < r1: (image, row, column) of a pixel index with
// (r1, r0) = (RH, RW); (tap row, tap column, channel) of a conv K index with (KW, SC).  Two digits: hi unused.
struct Mixed3 { int hi, mid, lo; };
OTAMD_HD Mixed3 mixed3_of(int v, int r1, int r0) {   // closed form
  const int t = v / r0, h = t / r1;
  return Mixed3{h, t - h * r1, v - t * r0};
}
OTAMD_HD Mixed3 mixed2_of(int v, int r0) {
  const int t = v / r0;
  return Mixed3{0, t, v - t * r0};
}
// a + d + e for e in {0, 1}: lo + d.lo + e < 2 r0 and mid + d.mid + 1 < 2 r1, so one conditional subtract per digit
OTAMD_HD Mixed3 mixed3_add(const Mixed3& a, const Mixed3& d, int e, int r1, int r0) {
  int lo = a.lo + d.lo + e;
  const int c0 = lo >= r0 ? 1 : 0;
  lo -= c0 ? r0 : 0;
  int mid = a.mid + d.mid + c0;
  const int c1 = mid >= r1 ? 1 : 0;
  mid -= c1 ? r1 : 0;
  return Mixed3{a.hi + d.hi + c1, mid, lo};
}
OTAMD_HD Mixed3 mixed2_add(const Mixed3& a, const Mixed3& d, int e, int r0) {
  int lo = a.lo + d.lo + e;
  const int c0 = lo >= r0 ? 1 : 0;
  lo -= c0 ? r0 : 0;
  return Mixed3{0, a.mid + d.mid + c0, lo};
}

// floor(x / d) as the high word of x * m, m = floor((2^32 - 1) / d) + 1: exact for 2 <= d and 0 <= x with x * d < 2^32
// (m d - 2^32 < d, so the error term x (m d - 2^32) / (2^32 d) stays below 1 / d); coordinates here are far below 2^16
OTAMD_HD unsigned recip_magic(int d) { return d >= 2 ? 0xFFFFFFFFu / (unsigned)d + 1u : 0u; }
OTAMD_HD int div_magic(int x, unsigned m) { return (int)(((unsigned long long)(unsigned)x * m) >> 32); }

// Per-lane DMA state of one operand tile (BMN rows/cols x 64 k): BMN/8 pieces of 1 KiB, NW waves
// take NI = BMN/(8 NW) each (piece j = wave + NW i).
template <int MODE, int BMN, int NW>
struct StageIndex {
  static constexpr bool KM = IsKMode<MODE>::v;
  static constexpr int NP = BMN / 8;                  // 1 KiB pieces per stage image
  static constexpr int NI = (NP + NW - 1) / NW;       // pieces per wave (the last may be absent)
  static constexpr bool EVEN = NP % NW == 0;          // 160-wide images: 20 pieces over 8 waves
  static constexpr int RB = BMN * 2;      // MN-mode row bytes
  static constexpr bool CONV = MODE >= OPM_CONV_FWD;  // the gathers with an incremental form
  // MN-mode: k rows between a lane's piece 0 and its piece i: UROWS(i), or UROWS(i) + 1 where pieces hold no whole
  // number of rows (160-wide images)
  static constexpr bool ROWS_EVEN = (NW * 1024) % RB == 0;
  static constexpr int UROWS(int i) { return NW * 1024 * i / RB; }
  // ... and where that distance is a multiple of 16 rows (the swizzle's period) every piece of a lane has the same
  // column: one (b, c, ok) serves all pieces
  static constexpr bool SAME_COL = ROWS_EVEN && (NI == 1 || UROWS(1) % 16 == 0);
  static constexpr int NEVER = 0x40000000;   // a coordinate no bound check passes (k, y < 2^30)
  int a[NI], b[NI], c[NI];                // K: (row elem offset | conv n,y0,x0) ; MN: (k row, col | tap offsets, ch)
  int t0, t1, t2;                         // K: logical chunk ; MN-conv: per-piece decode lives in a/b/c
  bool ok[NI];
  // incremental form.  cur, per lane: conv K-mode (tap row, tap column, channel) of this lane's k; wgrad (image, row,
  // column) and weight-read (-, tap, co) of the k row of piece 0.  d64 / du[i]: the digits of 64 and of UROWS(i)
  // (launch-uniform).  smagic: the dgrad stride's reciprocal (recip_magic).
  Mixed3 cur, d64, du[NI];
  unsigned smagic;

  OTAMD_HD void prepare(const ConvGeom& g, long long ld, int mn0, int MNsz, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int j = wave + NW * i;
      if constexpr (KM) {
        const int r = 8 * j + (lane >> 3);
        const int gm = mn0 + r;
        ok[i] = gm < MNsz;
        if constexpr (MODE == OPM_K) {
          a[i] = gm * (int)ld;
        } else {
          const int rr = ok[i] ? gm : 0;
          const int hw = g.RH * g.RW;
          const int n = rr / hw, rem = rr - n * hw;
          const int y = rem / g.RW, x = rem - y * g.RW;
          a[i] = n;
          if constexpr (MODE == OPM_CONV_FWD) { b[i] = y * g.stride - g.pad; c[i] = x * g.stride - g.pad; }
          else { b[i] = y + g.pad; c[i] = x + g.pad; }
        }
      } else {
        const int byte = j * 1024 + lane * 16;
        const int r = byte / RB;
        const int pc = (byte % RB) >> 4;
        const int lb = (pc >> 1) ^ mn_swz_rb<RB>(r);
        const int col = mn0 + (lb * 2 + (pc & 1)) * 8;
        a[i] = r;
        ok[i] = col < MNsz;
        if constexpr (MODE == OPM_MN || MODE == OPM_CONV_WT) {
          b[i] = col;
        } else {   // OPM_CONV_WGRAD: col = (tap, ch)
          const int cc = ok[i] ? col : 0;
          const int tap = cc / g.SC;
          c[i] = cc - tap * g.SC;
          b[i] = tap;
        }
      }
    }
    if constexpr (KM) t0 = (lane & 7) ^ ((lane >> 3) & 7);
    if constexpr (CONV) {
      if constexpr (KM) d64 = uniform(mixed3_of(64, g.KW, g.SC));
      else if constexpr (MODE == OPM_CONV_WGRAD) d64 = uniform(mixed3_of(64, g.RH, g.RW));
      else d64 = uniform(mixed2_of(64, g.SC));
      if constexpr (!KM) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
          du[i] = uniform(MODE == OPM_CONV_WGRAD ? mixed3_of(UROWS(i), g.RH, g.RW) : mixed2_of(UROWS(i), g.SC));
      }
      smagic = MODE == OPM_CONV_DGRAD ? OTAMD_UNIFORM(recip_magic(g.stride)) : 0u;
    }
  }
  static OTAMD_HD Mixed3 uniform(const Mixed3& m) {
    return Mixed3{OTAMD_UNIFORM(m.hi), OTAMD_UNIFORM(m.mid), OTAMD_UNIFORM(m.lo)};
  }
  // wgrad: the tap's offsets into the source, (tap row - pad) and (tap column - pad), as two 16-bit halves
  static OTAMD_HD int pack_tap(const ConvGeom& g, int tap) {
    const int tr = tap / g.KW, ts = tap - tr * g.KW;
    return (int)(((unsigned)(tr - g.pad) << 16) | ((unsigned)(ts - g.pad) & 0xffffu));
  }
  // k row of piece i inside the 64-deep K tile (MN modes)
  OTAMD_HD int krow(int i) const {
    if constexpr (CONV && ROWS_EVEN) return a[0] + UROWS(i);
    else return a[i];
  }

  // incremental form: the state of the split's first K tile (closed form, once per launch); offsets_step() must then
  // be called for k0 = kbeg, kbeg + 64, ... in order.  Also folds ok[] into a coordinate that fails its bound check
  // (conv K modes: the row y; MN modes with one column per lane: the k row), so the K loop keeps no validity flags.
  OTAMD_HD void start(const ConvGeom& g, int kbeg) {
    if constexpr (CONV) {
      if constexpr (KM) {
        cur = mixed3_of(kbeg + 8 * t0, g.KW, g.SC);
        cur.hi = (cur.hi << 3) | t0;   // the lane's chunk rides in the tap row's low bits: one register less in the loop
#pragma unroll
        for (int i = 0; i < NI; ++i) b[i] = ok[i] ? b[i] : -NEVER;
      } else if constexpr (MODE == OPM_CONV_WGRAD) {
        // a[i] becomes (k row | channel << 7 | NEVER where the column is outside): with b[i] two registers per piece
        cur = mixed3_of(kbeg + a[0], g.RH, g.RW);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          b[i] = pack_tap(g, b[i]);
          a[i] |= (c[i] << 7) | (ok[i] ? 0 : NEVER);
        }
      } else {
        cur = mixed2_of(kbeg + a[0], g.SC);
        if constexpr (SAME_COL) a[0] = ok[0] ? a[0] : NEVER;
      }
    }
  }
  // MN conv modes: piece i's column data (b, c, ok) and whether its column is inside the matrix
  static constexpr int ci(int i) { return SAME_COL ? 0 : i; }
  OTAMD_HD bool col_ok(int i) const { return SAME_COL ? true : ok[i]; }
  // wgrad's packed a[]: piece i's k row with the NEVER flag kept (for the k < Kend check), and its channel
  OTAMD_HD int wg_krow(int i) const {
    if constexpr (SAME_COL) return (a[0] & (NEVER | 127)) + UROWS(i);
    else return a[i] & (NEVER | 127);
  }
  OTAMD_HD int wg_ch(int i) const { return (a[ci(i)] >> 7) & 0x7fffff; }

  // flat source element (image n, row sy, column sx, channel ch) as a byte offset
  static OTAMD_HD unsigned src_off(const ConvGeom& g, int n, int sy, int sx, int ch) {
    return (unsigned)(((n * g.SH + sy) * g.SW + sx) * (int)g.ld + ch) * 2u;
  }

  // source byte offsets of this wave's pieces of the K tile at k0 (OFF_INVALID: zero-fill), incremental form; moves
  // the state on to k0 + 64
  OTAMD_HD void offsets_step(const ConvGeom& g, long long ld, int k0, int Kend, unsigned (&out)[NI]) {
    static_assert(CONV, "plain K / MN operands have no state: offsets()");
    if constexpr (KM) {
      const bool kok = k0 + 8 * (cur.hi & 7) < Kend;
      const int r_ = cur.hi >> 3, s_ = cur.mid, ch = cur.lo;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        unsigned off = OFF_INVALID;
        bool v = kok;   // a row past M has y = -NEVER
        int sy, sx;
        if constexpr (MODE == OPM_CONV_FWD) {
          const int y = b[i] + r_, x = c[i] + s_;
          if (g.upsample) { v = v && y >= 0 && y < 2 * g.SH && x >= 0 && x < 2 * g.SW; sy = y >> 1; sx = x >> 1; }
          else { v = v && y >= 0 && y < g.SH && x >= 0 && x < g.SW; sy = y; sx = x; }
        } else {
          const int ty = b[i] - r_, tx = c[i] - s_;
          if (g.stride == 1) { sy = ty; sx = tx; }
          else {   // ty, tx >= 0 where valid: the quotient by the stride's reciprocal, exact when it multiplies back
            sy = div_magic(ty, smagic); sx = div_magic(tx, smagic);
            v = v && ty >= 0 && tx >= 0 && (unsigned)sy * (unsigned)g.stride == (unsigned)ty &&
                (unsigned)sx * (unsigned)g.stride == (unsigned)tx;
          }
          v = v && sy >= 0 && sy < g.SH && sx >= 0 && sx < g.SW;
        }
        if (v) off = src_off(g, a[i], sy, sx, ch);
        out[i] = off;
      }
      const Mixed3 nx = mixed3_add(Mixed3{0, s_, ch}, Mixed3{0, d64.mid, d64.lo}, 0, g.KW, g.SC);   // nx.hi: the carry
      cur = Mixed3{cur.hi + ((d64.hi + nx.hi) << 3), nx.mid, nx.lo};
    } else if constexpr (MODE == OPM_CONV_WT) {   // k = tap*Cout + co -> W row co*KK + tap
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        unsigned off = OFF_INVALID;
        const Mixed3 t = i == 0 ? cur : mixed2_add(cur, du[i], ROWS_EVEN ? 0 : a[i] - a[0] - UROWS(i), g.SC);
        if (col_ok(i) && k0 + krow(i) < Kend) off = (unsigned)((t.lo * (g.KH * g.KW) + t.mid) * (int)ld + b[ci(i)]) * 2u;
        out[i] = off;
      }
      cur = mixed2_add(cur, d64, 0, g.SC);
    } else {   // conv wgrad: k = output pixel
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        unsigned off = OFF_INVALID;
        bool v = k0 + wg_krow(i) < Kend;
        const int bt = b[ci(i)];
        const Mixed3 px = i == 0 ? cur : mixed3_add(cur, du[i], ROWS_EVEN ? 0 : (a[i] & 127) - (a[0] & 127) - UROWS(i), g.RH, g.RW);
        const int y = px.mid * g.stride + (bt >> 16), x = px.lo * g.stride + (int)(short)(bt & 0xffff);
        int sy, sx;
        if (g.upsample) { v = v && y >= 0 && y < 2 * g.SH && x >= 0 && x < 2 * g.SW; sy = y >> 1; sx = x >> 1; }
        else { v = v && y >= 0 && y < g.SH && x >= 0 && x < g.SW; sy = y; sx = x; }
        if (v) off = src_off(g, px.hi, sy, sx, wg_ch(i));
        out[i] = off;
      }
      cur = mixed3_add(cur, d64, 0, g.RH, g.RW);
    }
  }

  // source byte offsets of this wave's pieces of the K tile at k0 (OFF_INVALID: zero-fill), closed form: the plain
  // K / MN operands, and the reference of the conv gathers (before start(): it reads the tap index in b[])
  OTAMD_HD void offsets(const ConvGeom& g, long long ld, int k0, int Kend, unsigned (&out)[NI]) const {
    if constexpr (KM) {
      const int k = k0 + 8 * t0;
      const bool kok = k < Kend;
      int r_ = 0, s_ = 0, ch = 0;
      if constexpr (MODE != OPM_K) {
        const int tap = kok ? k / g.SC : 0;
        ch = k - tap * g.SC;
        r_ = tap / g.KW;
        s_ = tap - r_ * g.KW;
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        unsigned off = OFF_INVALID;
        if constexpr (MODE == OPM_K) {
          if (kok && ok[i]) off = (unsigned)(a[i] + k) * 2u;
        } else {
          bool v = kok && ok[i];
          int sy, sx;
          if constexpr (MODE == OPM_CONV_FWD) {
            const int y = b[i] + r_, x = c[i] + s_;
            if (g.upsample) { v = v && y >= 0 && y < 2 * g.SH && x >= 0 && x < 2 * g.SW; sy = y >> 1; sx = x >> 1; }
            else { v = v && y >= 0 && y < g.SH && x >= 0 && x < g.SW; sy = y; sx = x; }
          } else {
            const int ty = b[i] - r_, tx = c[i] - s_;
            if (g.stride == 1) { sy = ty; sx = tx; }
            else {
              v = v && ty >= 0 && tx >= 0 && (ty % g.stride) == 0 && (tx % g.stride) == 0;
              sy = ty / g.stride; sx = tx / g.stride;
            }
            v = v && sy >= 0 && sy < g.SH && sx >= 0 && sx < g.SW;
          }
          if (v) off = (unsigned)(((a[i] * g.SH + sy) * g.SW + sx) * (int)g.ld + ch) * 2u;
        }
        out[i] = off;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int k = k0 + a[i];
        unsigned off = OFF_INVALID;
        if constexpr (MODE == OPM_MN) {
          if (ok[i] && k < Kend) off = (unsigned)(k * (int)ld + b[i]) * 2u;
        } else if constexpr (MODE == OPM_CONV_WT) {   // k = tap*Cout + co -> W row co*KK + tap
          if (ok[i] && k < Kend) {
            const int tap = k / g.SC, co = k - tap * g.SC;
            off = (unsigned)((co * (g.KH * g.KW) + tap) * (int)ld + b[i]) * 2u;
          }
        } else {   // conv wgrad: k = output pixel
          bool v = ok[i] && k < Kend;
          const int kk = v ? k : 0;
          const int hw = g.RH * g.RW;
          const int n = kk / hw, rem = kk - n * hw;
          const int p = rem / g.RW, q = rem - p * g.RW;
          const int tr = b[i] / g.KW, ts = b[i] - (b[i] / g.KW) * g.KW;
          const int y = p * g.stride - g.pad + tr, x = q * g.stride - g.pad + ts;
          int sy, sx;
          if (g.upsample) { v = v && y >= 0 && y < 2 * g.SH && x >= 0 && x < 2 * g.SW; sy = y >> 1; sx = x >> 1; }
          else { v = v && y >= 0 && y < g.SH && x >= 0 && x < g.SW; sy = y; sx = x; }
          if (v) off = (unsigned)(((n * g.SH + sy) * g.SW + sx) * (int)g.ld + c[i]) * 2u;
        }
        out[i] = off;
      }
    }
  }
};
