// The GEMM tile catalogue: the one host-side table of tile codes (gemm.hip's analytic planner and OTAMD_GEMM_TILE,
// gemm2.hip's launch geometry, gemm_plan.hip's fill rule and otamd_gemm_tile_dims all read it).
//
//   -1  v1 128x128 kernel of gemm.hip (4 waves, 2 workgroups per CU)
//    0  256x256     1  256x128     2  128x256     8 waves, 1 workgroup per CU, LDS-DMA
//    3  256x256 on 4 waves (explicit plans only)
//    4  128x128 on 8 waves, 2 workgroups per CU: the smallest epilogue; fills the chip on the 4096-row SDXL level-2
//       shapes where 256-wide tiles leave CUs idle (tools/gemm_tiles.py on MI355X: 4096x1280x1280 30.3 -> 26.2 us,
//       4096x10240x1280 129.5 -> 114.2 us, 4096x5120x1280 69.0 -> 60.0 us)
//    5  128x64      6  64x128      the skinny LoRA GEMMs (t = x A^T and u = dy B with N = rank, the adapter wgrads
//       with M or N = rank), where a 128- or 256-wide tile spends 2-8x the MFMA work on zero padding; three
//       workgroups per CU (48 KiB of LDS each)
//    7  128x160     8  256x160     N = 320 / 640 / 1280 without padding and 256 tiles for the 4096 x 1280 and
//       16384 x 640 shapes; rates fitted to the tools/gemm_tiles.py sweep of the SDXL step
//    9, 10  tiles 5, 6 on a 4-deep LDS ring (explicit plans and OTAMD_SKINNY_NS4 only)
//
// The template instances behind the codes are picked in gemm2_tiles_*.hip.
#pragma once

struct GemmTile {
  int code;
  const char* name;    // as accepted by OTAMD_GEMM_TILE (nullptr: not forcible)
  int bm, bn, waves, ring;
  // analytic-plan cost model (plan_gemm): workgroups per CU, per-CU throughput relative to the 256x256 tile
  // (tools/gemm_bench.py on MI355X), fixed prologue/epilogue seconds; candidate: the planner may choose the tile
  int per_cu;
  double rate, fixed;
  bool candidate;
};

static const GemmTile kGemmTiles[] = {
    {-1, "v1", 128, 128, 4, 0, 2, 0.55, 2.5e-6, true},       {0, "256x256", 256, 256, 8, 2, 1, 1.0, 2.5e-6, true},
    {1, "256x128", 256, 128, 8, 2, 1, 0.85, 2.5e-6, true},   {2, "128x256", 128, 256, 8, 2, 1, 0.85, 2.5e-6, true},
    {3, "256x256w4", 256, 256, 4, 2, 0, 0, 0, false},        {4, "128x128w8", 128, 128, 8, 2, 2, 0.85, 0.6e-6, true},
    {5, "128x64", 128, 64, 8, 2, 3, 0.55, 0.6e-6, true},     {6, "64x128", 64, 128, 8, 2, 3, 0.55, 0.6e-6, true},
    {7, "128x160", 128, 160, 8, 2, 2, 0.9, 4e-6, true},      {8, "256x160", 256, 160, 8, 2, 1, 0.9, 2.5e-6, true},
    {9, nullptr, 128, 64, 8, 4, 0, 0, 0, false},             {10, nullptr, 64, 128, 8, 4, 0, 0, 0, false}};
constexpr int kGemmTileMin = -1, kGemmTileMax = 10;

// the row of a tile code, nullptr outside the catalogue
inline const GemmTile* gemm_tile(int code) {
  return code < kGemmTileMin || code > kGemmTileMax ? nullptr : &kGemmTiles[code - kGemmTileMin];
}
