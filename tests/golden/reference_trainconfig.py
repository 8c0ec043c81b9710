"""Rebuild the reference's enum-typed TrainConfig objects from their record
(tests/golden/reference_trainconfigs.json, written by make_reference_trainconfigs.py).

    cfg, enums = reference_trainconfig("#sdxl 1.0.json")
    cfg.loss_scaler is enums["LossScaler"].NONE; cfg.optimizer.optimizer is enums["Optimizer"].ADAMW

Every enum-typed field holds a member of a real Enum class with the reference's member names and values, nested part
configs are objects with the reference's fields, so code that takes the reference's config object reads the same
attributes here.
"""
from __future__ import annotations

import json
from enum import Enum
from pathlib import Path
from types import SimpleNamespace

RECORD = Path(__file__).resolve().parent / "reference_trainconfigs.json"


def reference_trainconfig(preset: str):
    with open(RECORD) as f:
        rec = json.load(f)
    enums = {name: Enum(name, members) for name, members in rec["enums"].items()}

    def build(v):
        if isinstance(v, dict) and set(v) == {"__enum__", "name"}:
            return enums[v["__enum__"]][v["name"]]
        if isinstance(v, dict) and set(v) == {"__config__"}:
            return SimpleNamespace(**{k: build(x) for k, x in v["__config__"].items()})
        if isinstance(v, list):
            return [build(x) for x in v]
        if isinstance(v, dict):
            return {k: build(x) for k, x in v.items()}
        return v

    return build(rec["configs"][preset]), enums
