"""Plan resolution in libotamd (csrc/gemm_plan.hip) against the decisions recorded before it moved there
(tests/golden/gemm_plan_census.json, lora_fused_census.json; made by tests/golden/make_plan_census.py): the same
(tile, splits) for every signature of the measured table -- with the table, with the analytic planner alone and at
explicit splits -- and the same fused / two-launch decision over the LoRA site grid.  Integers: exact.  Host code
only, no GPU."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from onetrainer_amd import kernels as K

GOLD = Path(__file__).parent / "golden"
sys.path.insert(0, str(GOLD))
import make_plan_census as MC  # noqa: E402


def _resolve(a, splits):
    tile, s = C.c_int(-9), C.c_int(-9)
    wb = K._planner().otamd_gemm_resolve(C.byref(a), splits, C.byref(tile), C.byref(s))
    assert wb == K._ws_bytes(a, s.value)
    return [tile.value, s.value]


@pytest.fixture
def no_plan_table():
    """the library with an empty measured plan table; the loaded one is put back afterwards"""
    lib = K._planner()
    assert lib.otamd_gemm_set_plan_table(None, 0) == 0 and lib.otamd_gemm_plan_table_size() == 0
    yield
    K._PLANNER = None
    assert K._planner().otamd_gemm_plan_table_size() == len(K._plan_table())


def test_gemm_plans_with_table():
    rows = json.loads((GOLD / "gemm_plan_census.json").read_text())["rows"]
    assert {tuple(r["key"]) for r in rows} == set(K._plan_table())
    for r in rows:
        a = MC.gemm_args(r["key"])
        assert list(K._tune_key(a)) == r["key"]
        assert _resolve(a, 0) == r["table"], r["key"]
        for s, want in r["splits"].items():
            assert _resolve(a, int(s)) == want, (r["key"], s)


def test_gemm_plans_analytic(no_plan_table):
    for r in json.loads((GOLD / "gemm_plan_census.json").read_text())["rows"]:
        assert _resolve(MC.gemm_args(r["key"]), 0) == r["analytic"], r["key"]


def test_lora_fused_decisions():
    sites = json.loads((GOLD / "lora_fused_census.json").read_text())["sites"]
    assert [tuple(s[:5]) for s in sites] == MC.lora_sites()
    lib = K._planner()
    for form, N, Kd, parts, M, lp, fused, fused_bias in sites:
        assert K._lora_plan(form, N, Kd, parts, M) == lp, (form, N, Kd, parts, M)
        for bias, want in ((False, fused), (True, fused_bias)):
            a = MC.lora_base(form, N, Kd, parts, M, bias)
            assert lib.otamd_lora_fused_tile(C.byref(a), form, parts) == want, (form, N, Kd, parts, M, bias)


def test_tile_dims():
    """every catalogue row; tiles 5-8 as lora_plans_mi355x.json's entries and kernels._skinny_split assume them"""
    dims = {-1: (128, 128), 0: (256, 256), 1: (256, 128), 2: (128, 256), 3: (256, 256), 4: (128, 128), 5: (128, 64),
            6: (64, 128), 7: (128, 160), 8: (256, 160), 9: (128, 64), 10: (64, 128)}
    for tile, want in dims.items():
        assert K._tile_dims(tile) == want, tile
    bm, bn = C.c_int(0), C.c_int(0)
    for tile in (-2, 11):
        assert K.lib().otamd_gemm_tile_dims(tile, C.byref(bm), C.byref(bn)) == 1
