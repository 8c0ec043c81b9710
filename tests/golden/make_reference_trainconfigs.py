"""Record the reference's enum-typed TrainConfig objects for the C1-C5 training presets (data only).

    python tests/golden/make_reference_trainconfigs.py <reference checkout>
        -> tests/golden/reference_trainconfigs.json, tests/golden/training_presets/*.json

The reference's TrainConfig.default_values().from_dict(<preset>) is walked field by field (BaseConfig.types):
an Enum member is stored as {"__enum__": <class name>, "name": <member name>}, a nested BaseConfig as
{"__config__": {field: ...}}, everything else as its JSON value.  "enums" lists every member (name -> value) of each
Enum class met, so a test can rebuild the object with real Enum members in every enum field
(tests/test_config_boundary.py, tests/test_dtype_policy.py: reference_trainconfig()).  The preset files
tests/test_host_logic.py loads are copied next to it unchanged (they hold settings only).
"""
from __future__ import annotations

import json
import shutil
import sys
from enum import Enum
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "reference_trainconfigs.json"
PRESETS = ["#sd 1.5.json", "#sdxl 1.0.json", "#sdxl 1.0 LoRA.json", "#flux LoRA.json"]
COPIED = ["#sdxl 1.0.json", "#sdxl 1.0 LoRA.json"]


def main(ref: Path):
    sys.path.insert(0, str(ref))
    from modules.util.config.TrainConfig import TrainConfig
    enums = {}

    def node(v):
        if isinstance(v, Enum):
            cls = type(v)
            enums.setdefault(cls.__name__, {m.name: m.value for m in cls})
            return {"__enum__": cls.__name__, "name": v.name}
        if hasattr(v, "to_dict") and hasattr(v, "types"):
            return {"__config__": {k: node(getattr(v, k)) for k in v.types}}
        if isinstance(v, (list, tuple)):
            return [node(x) for x in v]
        if isinstance(v, dict):
            return {str(k): node(x) for k, x in v.items()}
        json.dumps(v)   # plain data only
        return v

    configs = {}
    for fname in PRESETS:
        c = TrainConfig.default_values()
        with open(ref / "training_presets" / fname) as f:
            c.from_dict(json.load(f))
        configs[fname] = node(c)
    json.dumps(enums)
    with open(OUT, "w") as f:
        json.dump({"enums": enums, "configs": configs}, f, indent=0)
    (HERE / "training_presets").mkdir(exist_ok=True)
    for fname in COPIED:
        shutil.copyfile(ref / "training_presets" / fname, HERE / "training_presets" / fname)
    print("wrote", OUT, len(configs), "configs,", len(enums), "enum classes")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
