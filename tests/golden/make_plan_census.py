"""Record the GEMM planner's decisions as fixtures (tests/test_plan_census.py replays them through libotamd):

  gemm_plan_census.json    the (tile, splits) every signature of gemm_plans_mi355x.json launches on -- with the
                           measured table, with the analytic planner alone, and at explicit splits 1 / 2 / 4
  lora_fused_census.json   over a grid of LoRA sites: the fused-LoRA table's answer and the tile the site launches
                           fused on (0: two launches)

    python tests/golden/make_plan_census.py          (needs the built library and host layer; no GPU)

Run it at the commit whose plans are to be pinned.  It restates how the host layer combines the tables and the
analytic planner from their parts (the table dict, h.lora_plan, otamd_gemm_plan, otamd_gemm_plan_tile), so a later
change of that combination shows against the record.  The committed files were recorded at d9a398d, before plan
resolution moved into the library.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from onetrainer_amd import kernels as K  # noqa: E402
from onetrainer_amd._lib import GemmArgs, lib  # noqa: E402

PTR = 0x10000   # a 16-byte aligned non-null operand address (nothing is launched)
SPLITS = (1, 2, 4)
LORA_GRID = {"forms": (0, 1), "N": (640, 1280, 1920, 2560, 3840, 5120, 10240),
             "K": (640, 1280, 1920, 2560, 3840, 5120, 10240), "parts": (1, 3),
             "M": (4, 4032, 4096, 4160, 16128, 16384, 16640, 65536)}


def gemm_args(key) -> GemmArgs:
    """GemmArgs with the signature `key` (the plan table's 16 fields)"""
    am, bm, M, N, Kd, K1, batch, c_f32, bias, rowvec, residual, acc, ga_kh, ga_stride, ga_up, gb_kh = key
    a = GemmArgs()
    a.alpha, a.rows_per_vec = 1.0, 1
    a.A = a.B = a.C = PTR
    a.amode, a.bmode, a.M, a.N, a.K, a.batch, a.bdiv, a.c_f32, a.accumulate = am, bm, M, N, Kd, batch, 1, c_f32, acc
    a.bias, a.rowvec, a.residual = (PTR if bias else None), (PTR if rowvec else None), (PTR if residual else None)
    a.ga.KH, a.ga.stride, a.ga.upsample, a.gb.KH = ga_kh, ga_stride, ga_up, gb_kh
    if K1:
        a.A2 = a.B2 = PTR
        a.K1, a.K2 = K1, Kd - K1
    return a


def lora_base(form: int, N: int, Kd: int, parts: int, M: int, bias: bool) -> GemmArgs:
    """the two-launch form's base GEMM of a LoRA site: the linear forward (form 0) or input gradient (form 1) with
    the rank-32-per-part adapter product attached as the second K segment"""
    return gemm_args((0, form, M, N, Kd + 32 * parts, Kd, 0, 0, int(bias), 0, 0, 0, 0, 0, 0, 0))


def lora_sites():
    g = LORA_GRID
    return [(f, N, Kd, p, M) for f in g["forms"] for N in g["N"] for Kd in g["K"] for p in g["parts"] for M in g["M"]]


def _analytic(a: GemmArgs, splits: int):
    s = C.c_int(0)
    assert lib().otamd_gemm_plan(C.byref(a), splits, C.byref(s)) >= 0
    return [lib().otamd_gemm_plan_tile(C.byref(a), s.value), s.value]


def _fused_tile(h, table, a: GemmArgs, form: int, parts: int) -> int:
    lp = h.lora_plan(form, a.N, a.K1, parts, a.M)
    if lp:
        return max(lp, 0)
    plan = table.get(K._tune_key(a))
    if plan is None:
        s = C.c_int(0)
        if lib().otamd_gemm_plan(C.byref(a), 0, C.byref(s)) < 0:
            return 0
        plan = (lib().otamd_gemm_plan_tile(C.byref(a), 0), s.value)
    tile, splits = plan
    return 0 if splits != 1 else (tile or 4)


def main():
    table, h = K._plan_table(), K._host()
    assert table and h is not None
    rows = []
    for key in sorted(table):
        a = gemm_args(key)
        rows.append({"key": list(key), "table": list(table[key]), "analytic": _analytic(a, 0),
                     "splits": {str(s): _analytic(a, s) for s in SPLITS}})
    with open(os.path.join(HERE, "gemm_plan_census.json"), "w") as f:
        json.dump({"rows": rows}, f, separators=(",", ":"))
    sites = []
    for form, N, Kd, parts, M in lora_sites():
        fused = [_fused_tile(h, table, lora_base(form, N, Kd, parts, M, b), form, parts) for b in (False, True)]
        sites.append([form, N, Kd, parts, M, h.lora_plan(form, N, Kd, parts, M)] + fused)
    with open(os.path.join(HERE, "lora_fused_census.json"), "w") as f:
        json.dump({"columns": "form, N, K, parts, M, lora_plan, fused tile without bias, fused tile with bias",
                   "sites": sites}, f, separators=(",", ":"))
    print(len(rows), "signatures,", len(sites), "LoRA sites")


if __name__ == "__main__":
    main()
