// GEMM plan resolution (host code only): which (tile, split-K) a GEMM launches on and whether a LoRA site runs fused,
// for both host paths (csrc/host/ops_host.cpp and kernels.py).  Measured tables first -- the plan table
// (gemm_plans_mi355x.json) and the fused-LoRA tile table (lora_plans_mi355x.json), loaded by kernels.py and stored
// here -- then gemm.hip's analytic planner.
#include "gemm.h"
#include "gemm_tiles.h"

#include <array>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>
#include <utility>

OTAMD_API long long otamd_gemm_plan(const GemmArgs* in, int splits, int* splits_out);   // gemm.hip
OTAMD_API int otamd_gemm_plan_tile(const GemmArgs* in, int splits);
OTAMD_API long long otamd_gemm_ws_bytes(const GemmArgs* in, int splits);

namespace {

using PlanKey = std::array<long long, 16>;
struct PlanHash {
  size_t operator()(const PlanKey& k) const {
    size_t h = 1469598103934665603ULL;
    for (long long v : k) h = (h ^ (size_t)v) * 1099511628211ULL;
    return h;
  }
};
// The library's launchers are thread-compatible; these two tables are read per GEMM (shared lock) and written only
// when a table is loaded (exclusive lock).
std::shared_mutex g_mu;
std::unordered_map<PlanKey, std::pair<int, int>, PlanHash> g_plans;   // signature -> (tile, splits)
std::map<std::array<long long, 5>, int> g_lora_plans;   // (form, N, K, parts, M class or -M) -> tile, -1: two launches

PlanKey plan_key(const GemmArgs& a) {
  return {a.amode, a.bmode, a.M, a.N, a.K, a.A2 ? a.K1 : 0, a.batch, a.c_f32, a.bias != nullptr, a.rowvec != nullptr,
          a.residual != nullptr, a.accumulate, a.ga.KH, a.ga.stride, a.ga.upsample, a.gb.KH};
}

bool measured_plan(const GemmArgs& a, int* tile, int* splits) {
  const PlanKey k = plan_key(a);
  std::shared_lock<std::shared_mutex> lk(g_mu);
  auto it = g_plans.find(k);
  if (it == g_plans.end()) return false;
  *tile = it->second.first;
  *splits = it->second.second;
  return true;
}

}  // namespace

OTAMD_API int otamd_gemm_tile_dims(int tile, int* bm, int* bn) {
  const GemmTile* t = gemm_tile(tile);
  if (!t || !bm || !bn) return OTAMD_EINVAL;
  *bm = t->bm;
  *bn = t->bn;
  return OTAMD_OK;
}

// the signature a measured plan is keyed by: amode, bmode, M, N, K, K1, batch, c_f32, bias, rowvec, residual,
// accumulate, ga.KH, ga.stride, ga.upsample, gb.KH
OTAMD_API int otamd_gemm_plan_key(const GemmArgs* in, long long key[16]) {
  if (!in || !key) return OTAMD_EINVAL;
  const PlanKey k = plan_key(*in);
  for (int i = 0; i < 16; ++i) key[i] = k[i];
  return OTAMD_OK;
}

// replace the measured plan table: n rows of 18 (the 16 key fields, tile, splits)
OTAMD_API int otamd_gemm_set_plan_table(const long long* rows, int n) {
  if (n < 0 || (n && !rows)) return OTAMD_EINVAL;
  decltype(g_plans) table;
  for (int i = 0; i < n; ++i) {
    const long long* r = rows + 18 * i;
    if (!gemm_tile((int)r[16]) || r[17] < 1) return OTAMD_EINVAL;
    PlanKey k;
    for (int j = 0; j < 16; ++j) k[j] = r[j];
    table[k] = {(int)r[16], (int)r[17]};
  }
  std::unique_lock<std::shared_mutex> lk(g_mu);
  g_plans.swap(table);
  return OTAMD_OK;
}

OTAMD_API int otamd_gemm_plan_table_size(void) {
  std::shared_lock<std::shared_mutex> lk(g_mu);
  return (int)g_plans.size();
}

// replace the fused-LoRA tile table: n rows of 6 (form, N, K, parts, M class -- or -M for an exact row count --, tile)
OTAMD_API int otamd_lora_set_plans(const long long* rows, int n) {
  if (n < 0 || (n && !rows)) return OTAMD_EINVAL;
  decltype(g_lora_plans) table;
  for (int i = 0; i < n; ++i) {
    const long long* r = rows + 6 * i;
    table[{r[0], r[1], r[2], r[3], r[4]}] = (int)r[5];
  }
  std::unique_lock<std::shared_mutex> lk(g_mu);
  g_lora_plans.swap(table);
  return OTAMD_OK;
}

// the plan to pass to otamd_gemm_explicit and its workspace bytes (< 0: invalid arguments).  splits == 0: the measured
// plan, else the analytic one; splits > 0: the analytic tile for that split count.
OTAMD_API long long otamd_gemm_resolve(const GemmArgs* in, int splits, int* tile, int* splits_out) {
  if (!in || !tile || !splits_out) return -1;
  if (splits == 0 && measured_plan(*in, tile, splits_out)) return otamd_gemm_ws_bytes(in, *splits_out);
  const long long wb = otamd_gemm_plan(in, splits, splits_out);
  if (wb >= 0) *tile = otamd_gemm_plan_tile(in, *splits_out);
  return wb;
}

// The measured fused-LoRA tile of a site (form 0: forward y = x W^T + t up^T, 1: input gradient; N, K of the base GEMM,
// adapter parts, M rows): > 0 the tile, -1 two launches, 0 no entry (the two-launch form's plan decides).
// The entries were measured at M = 4096 / 16384 (one tile per CU or whole waves of them); at the aspect buckets' other
// row counts a tile grid just past a multiple of the 256 CUs runs a second round for a few tiles (4160 rows on
// 128x160 tiles: 264 tiles, ~2x the time), so an entry applies only while the grid fills its rounds >= 85 %.
// An entry for the exact row count (class slot = -M: the aspect buckets' rows, measured) comes first, unchecked.
OTAMD_API int otamd_lora_plan(int form, int N, int K, int parts, int M) {
  int tile = 0;
  {
    std::shared_lock<std::shared_mutex> lk(g_mu);
    auto ex = g_lora_plans.find({form, N, K, parts, -(long long)M});
    if (ex != g_lora_plans.end()) return ex->second;
    auto it = g_lora_plans.find({form, N, K, parts, M >= 8192 ? 1 : 0});
    if (it == g_lora_plans.end()) return 0;
    tile = it->second;
  }
  if (tile <= 0) return tile;
  const GemmTile* t = gemm_tile(tile);
  if (!t) return 0;
  const long long tiles = (long long)((M + t->bm - 1) / t->bm) * ((N + t->bn - 1) / t->bn);
  const long long rounds = (tiles + 255) / 256;
  return tiles * 100 >= rounds * 256 * 85 ? tile : 0;
}

// The tile a LoRA site launches fused on, or 0 for the two launches.  base: the two-launch form's base GEMM (second K
// segment attached, K1 = the base K).  The LoRA table's entry first (linear forms only); without one the plan of
// `base` -- measured, else analytic -- and the site is fused only when that plan is one split.
OTAMD_API int otamd_lora_fused_tile(const GemmArgs* base, int form, int parts) {
  if (!base) return 0;
  const int lp = (form == 1 || base->amode == OPM_K) ? otamd_lora_plan(form, base->N, base->K1, parts, base->M) : 0;
  if (lp != 0) return lp > 0 ? lp : 0;
  int tile = 0, splits = 0;
  if (!measured_plan(*base, &tile, &splits)) {
    tile = otamd_gemm_plan_tile(base, 0);
    if (otamd_gemm_plan(base, 0, &splits) < 0) return 0;
  }
  if (splits != 1 || tile < 0) return 0;
  return tile == 0 ? 4 : tile;   // no fused 256x256 instance (register cap): the 128x128 tile
}
