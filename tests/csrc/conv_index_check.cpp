// Host check of the conv gather index decode (onetrainer_amd/csrc/gemm2_stage.h): for a sweep of conv geometries,
// every operand mode with an incremental form, every tile width, wave, lane and DMA piece, the offsets that
// offsets_step() carries from K-step to K-step must equal the closed (division) form offsets() at every K-step of
// every split, OFF_INVALID (zero-fill) lanes included.  Prints the number of compared offsets; exits 1 at the first
// difference.  Built by tests/test_conv_index.py, once plain and once with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "gemm2_stage.h"

static long long n_cmp = 0, n_valid = 0, n_steps = 0;

struct Split { int kbeg, kend; };

template <int MODE, int BMN, int NW>
static void walk(const ConvGeom& g, long long ld, int MNsz, int K, const char* what) {
  using S = StageIndex<MODE, BMN, NW>;
  // splits as the launcher cuts them (whole 64-deep K-steps): all of K; from 64 (inside a tap when SC is no divisor
  // of 64, inside an image row when RW is none); a middle split of three K-steps from 128
  const Split splits[] = {{0, K}, {64, K}, {128, K < 320 ? K : 320}};
  const int tiles = (MNsz + BMN - 1) / BMN;
  for (int tile = 0; tile < tiles; tile += (tiles > 1 ? tiles - 1 : 1)) {   // the first and the last (ragged) tile
    for (const Split& sp : splits) {
      if (sp.kbeg >= sp.kend) continue;
      for (int wave = 0; wave < NW; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
          S ref, inc;
          ref.prepare(g, ld, tile * BMN, MNsz, wave, lane);
          inc.prepare(g, ld, tile * BMN, MNsz, wave, lane);
          inc.start(g, sp.kbeg);
          for (int k0 = sp.kbeg; k0 < sp.kend; k0 += 64) {
            unsigned want[S::NI], got[S::NI];
            ref.offsets(g, ld, k0, sp.kend, want);
            inc.offsets_step(g, ld, k0, sp.kend, got);
            ++n_steps;
            for (int i = 0; i < S::NI; ++i) {
              ++n_cmp;
              n_valid += want[i] != OFF_INVALID;
              if (want[i] != got[i]) {
                std::printf("MISMATCH %s tile %dx%d waves: N %d S %dx%dx%d R %dx%d k %dx%d stride %d pad %d up %d | mn0 %d "
                            "split [%d, %d) k0 %d wave %d lane %d piece %d: closed %#x incremental %#x\n",
                            what, BMN, NW, g.N, g.SH, g.SW, g.SC, g.RH, g.RW, g.KH, g.KW, g.stride, g.pad, g.upsample,
                            tile * BMN, sp.kbeg, sp.kend, k0, wave, lane, i, want[i], got[i]);
                std::exit(1);
              }
            }
          }
        }
    }
  }
}

template <int MODE>
static void walk_tiles(const ConvGeom& g, long long ld, int MNsz, int K, const char* what) {
  walk<MODE, 256, 8>(g, ld, MNsz, K, what);
  walk<MODE, 256, 4>(g, ld, MNsz, K, what);
  walk<MODE, 128, 8>(g, ld, MNsz, K, what);
  walk<MODE, 64, 8>(g, ld, MNsz, K, what);
  if constexpr (!IsKMode<MODE>::v) walk<MODE, 160, 8>(g, ld, MNsz, K, what);   // 160-wide images: B operands only
}

static ConvGeom geom(int N, int SH, int SW, int SC, int RH, int RW, int k, int stride, int pad, int up, long long ld) {
  ConvGeom g;
  g.N = N; g.SH = SH; g.SW = SW; g.SC = SC; g.RH = RH; g.RW = RW; g.KH = k; g.KW = k;
  g.stride = stride; g.pad = pad; g.upsample = up; g.pad_ = 0; g.ld = ld;
  return g;
}

int main() {
  const int RWs[] = {1, 5, 7, 32, 70}, RHs[] = {3, 10};   // R = RH x RW pixels: 3 .. 700, below and above 64
  const int Ns[] = {1, 3}, SCs[] = {8, 64, 72, 192}, Ks[] = {1, 3};
  struct { int stride, up; } const forms[] = {{1, 0}, {2, 0}, {3, 0}, {1, 1}};
  for (int RW : RWs) for (int RH : RHs) for (int N : Ns) for (int SC : SCs) for (int k : Ks) for (auto f : forms) {
    const int pad = k / 2, st = f.stride;
    const int other = SC == 72 ? 40 : 72;   // the channel count of the other tensor (no multiple of the tile)
    {   // forward and weight gradient: R = the output P x Q, the source is the (upsampled) input
      const int H = (RH - 1) * st + k - 2 * pad, W = (RW - 1) * st + k - 2 * pad;   // virtual input size
      const int SH = f.up ? (H + 1) / 2 : H, SW = f.up ? (W + 1) / 2 : W;
      const ConvGeom g = geom(N, SH, SW, SC, RH, RW, k, st, pad, f.up, SC + 8);     // ld: a channel slice of a wider tensor
      walk_tiles<OPM_CONV_FWD>(g, 0, N * RH * RW, k * k * SC, "conv fwd A");
      walk_tiles<OPM_CONV_WGRAD>(g, 0, k * k * SC, N * RH * RW, "conv wgrad B");
    }
    if (!f.up) {   // input gradient: R = the input H x W, the source is dy [N, P, Q, Cout = SC]; B is the stored weight
      const int P = (RH + 2 * pad - k) / st + 1, Q = (RW + 2 * pad - k) / st + 1;
      const ConvGeom g = geom(N, P, Q, SC, RH, RW, k, st, pad, 0, SC);
      walk_tiles<OPM_CONV_DGRAD>(g, 0, N * RH * RW, k * k * SC, "conv dgrad A");
      const ConvGeom gb = geom(N, P, Q, SC, RH, RW, k, st, pad, 0, other);
      walk_tiles<OPM_CONV_WT>(gb, other, other, k * k * SC, "conv dgrad B (stored weight)");
    }
  }
  std::printf("conv index: %lld offsets over %lld K-steps equal in both forms (%lld valid, %lld zero-fill)\n", n_cmp,
              n_steps, n_valid, n_cmp - n_valid);
  return (n_valid > 0 && n_valid < n_cmp) ? 0 : 1;
}
