// Host check of the conv gathers under circular padding (onetrainer_amd/csrc/gemm2_stage.h, ConvGeom.circular): for a
// short sweep of small geometries, every wave, lane and DMA piece of the closed form offsets() and of the incremental
// form offsets_step(), at every K-step, must equal a brute-force decode written from the definition: a forward /
// weight-gradient tap coordinate y = p stride + r - pad in [-pad, 0) reads y + H, in [H, H + pad) reads y - H, anything
// else outside [0, H) is zero; the input gradient takes, for each (pixel, tap), the output pixel whose wrapped forward
// coordinate is that pixel.  Exits 1 at the first difference.  Built by tests/test_conv_circular_index.py, once plain
// and once with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "gemm2_stage.h"

static long long n_cmp = 0, n_wrapped = 0, n_zero = 0;

// the definition; -1: zero-fill.  wrapped: the coordinate came from the other edge
static int wrap_def(int y, int H, int pad, bool& wrapped) {
  if (y >= 0 && y < H) return y;
  wrapped = true;
  if (y >= -pad && y < 0) return y + H;
  if (y >= H && y < H + pad) return y - H;
  return -1;
}
static unsigned flat(const ConvGeom& g, int n, int sy, int sx, int ch) {
  return (unsigned)(((n * g.SH + sy) * g.SW + sx) * (int)g.ld + ch) * 2u;
}
// forward / weight gradient: output pixel (n, p, q), tap (r, s), channel ch
static unsigned expect_fwd(const ConvGeom& g, int n, int p, int q, int r, int s, int ch) {
  const int f = g.upsample ? 2 : 1;
  bool w = false;
  const int y = wrap_def(p * g.stride + r - g.pad, f * g.SH, g.pad, w);
  const int x = wrap_def(q * g.stride + s - g.pad, f * g.SW, g.pad, w);
  if (y < 0 || x < 0) return OFF_INVALID;
  n_wrapped += w;
  return flat(g, n, y / f, x / f, ch);
}
// the output coordinate p in [0, P) with wrap(p stride + r - pad) == h, or -1; at most one exists
static int adjoint(int h, int r, int H, int P, int stride, int pad, bool& wrapped) {
  int found = -1;
  for (int p = 0; p < P; ++p) {
    bool w = false;
    if (wrap_def(p * stride + r - pad, H, pad, w) != h) continue;
    if (found >= 0) { std::printf("two sources for one (pixel, tap): h %d r %d H %d\n", h, r, H); std::exit(1); }
    found = p;
    wrapped = wrapped || w;
  }
  return found;
}
static unsigned expect_dgrad(const ConvGeom& g, int n, int h, int w_, int r, int s, int co) {
  bool w = false;
  const int p = adjoint(h, r, g.RH, g.SH, g.stride, g.pad, w), q = adjoint(w_, s, g.RW, g.SW, g.stride, g.pad, w);
  if (p < 0 || q < 0) return OFF_INVALID;
  n_wrapped += w;
  return flat(g, n, p, q, co);
}

// what lane `lane` of piece j fetches at k0, from the tile layout alone (StageIndex::prepare)
template <int MODE, int BMN>
static unsigned expect(const ConvGeom& g, int MNsz, int k0, int Kend, int j, int lane) {
  int mn, k;
  if (IsKMode<MODE>::v) {
    mn = 8 * j + (lane >> 3);
    k = k0 + 8 * ((lane & 7) ^ ((lane >> 3) & 7));
  } else {
    constexpr int RB = BMN * 2;
    const int byte = j * 1024 + lane * 16, kr = byte / RB, pc = (byte % RB) >> 4;
    mn = (((pc >> 1) ^ mn_swz_rb<RB>(kr)) * 2 + (pc & 1)) * 8;
    k = k0 + kr;
  }
  if (mn >= MNsz || k >= Kend) return OFF_INVALID;
  const int pix = IsKMode<MODE>::v ? mn : k, kc = IsKMode<MODE>::v ? k : mn;   // the pixel index and the (tap, channel)
  const int n = pix / (g.RH * g.RW), a = pix / g.RW % g.RH, b = pix % g.RW;
  const int tap = kc / g.SC, ch = kc % g.SC, r = tap / g.KW, s = tap % g.KW;
  return MODE == OPM_CONV_DGRAD ? expect_dgrad(g, n, a, b, r, s, ch) : expect_fwd(g, n, a, b, r, s, ch);
}

template <int MODE, int BMN, int NW>
static void walk(const ConvGeom& g, int MNsz, int K, const char* what) {
  using S = StageIndex<MODE, BMN, NW>;
  for (int kbeg = 0; kbeg <= 64 && kbeg < K; kbeg += 64)   // one split, and a split that starts inside a tap / row
    for (int wave = 0; wave < NW; ++wave)
      for (int lane = 0; lane < 64; ++lane) {
        S ref, inc;
        ref.prepare(g, 0, 0, MNsz, wave, lane);
        inc.prepare(g, 0, 0, MNsz, wave, lane);
        inc.start(g, kbeg);
        for (int k0 = kbeg; k0 < K; k0 += 64) {
          unsigned closed[S::NI], step[S::NI];
          ref.offsets(g, 0, k0, K, closed);
          inc.offsets_step(g, 0, k0, K, step);
          for (int i = 0; i < S::NI; ++i) {
            if (wave + NW * i >= S::NP) continue;
            const unsigned want = expect<MODE, BMN>(g, MNsz, k0, K, wave + NW * i, lane);
            ++n_cmp;
            n_zero += want == OFF_INVALID;
            if (closed[i] != want || step[i] != want) {
              std::printf("MISMATCH %s tile %dx%d waves: N %d S %dx%dx%d R %dx%d stride %d pad %d up %d | split from %d k0 %d "
                          "wave %d lane %d piece %d: definition %#x closed %#x incremental %#x\n",
                          what, BMN, NW, g.N, g.SH, g.SW, g.SC, g.RH, g.RW, g.stride, g.pad, g.upsample, kbeg, k0, wave,
                          lane, i, want, closed[i], step[i]);
              std::exit(1);
            }
          }
        }
      }
}

template <int MODE>
static void walk_tiles(const ConvGeom& g, int MNsz, int K, const char* what) {
  walk<MODE, 256, 4>(g, MNsz, K, what);
  walk<MODE, 128, 8>(g, MNsz, K, what);
  walk<MODE, 64, 8>(g, MNsz, K, what);
  if constexpr (!IsKMode<MODE>::v) walk<MODE, 160, 8>(g, MNsz, K, what);
}

static ConvGeom geom(int N, int SH, int SW, int SC, int RH, int RW, int stride, int pad, int up) {
  ConvGeom g;
  g.N = N; g.SH = SH; g.SW = SW; g.SC = SC; g.RH = RH; g.RW = RW; g.KH = 3; g.KW = 3;
  g.stride = stride; g.pad = pad; g.upsample = up; g.circular = 1; g.ld = SC + 8;
  return g;
}

int main() {
  const int N = 2, k = 3;
  const int HW[][2] = {{1, 1}, {2, 2}, {3, 5}, {4, 6}};   // odd and even sizes under stride 2
  struct { int stride, up; } const forms[] = {{1, 0}, {2, 0}, {1, 1}};
  for (auto hw : HW) for (int SC : {8, 72}) for (auto f : forms) {
    const int H = hw[0], W = hw[1], u = f.up ? 2 : 1;
    const int P = (u * H + 2 - k) / f.stride + 1, Q = (u * W + 2 - k) / f.stride + 1;
    const ConvGeom g = geom(N, H, W, SC, P, Q, f.stride, 1, f.up);
    walk_tiles<OPM_CONV_FWD>(g, N * P * Q, k * k * SC, "conv fwd A");
    walk_tiles<OPM_CONV_WGRAD>(g, k * k * SC, N * P * Q, "conv wgrad B");
    if (!f.up) walk_tiles<OPM_CONV_DGRAD>(geom(N, P, Q, SC, H, W, f.stride, 1, 0), N * H * W, k * k * SC, "conv dgrad A");
  }
  {   // pad 0, stride 2, one output row / column more than computed (the VAE Downsample2D form): the last ones read zeros
    const long long zero0 = n_zero;
    const ConvGeom g = geom(N, 4, 6, 8, 2, 3, 2, 0, 0);
    walk_tiles<OPM_CONV_FWD>(g, N * 2 * 3, k * k * 8, "conv fwd A, pad 0");
    walk_tiles<OPM_CONV_WGRAD>(g, k * k * 8, N * 2 * 3, "conv wgrad B, pad 0");
    if (n_zero == zero0) return 1;
  }
  std::printf("conv circular: %lld offsets equal the definition in both forms (%lld wrapped, %lld zero-fill)\n", n_cmp,
              n_wrapped, n_zero);
  return n_wrapped > 0 ? 0 : 1;
}
