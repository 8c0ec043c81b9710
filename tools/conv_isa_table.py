"""Static table of the conv-gather instances of gemm2_kernel: registers, scratch, occupancy and the K-loop's instruction mix.

    python tools/conv_isa_table.py --csrc onetrainer_amd/csrc --out new.csv
    python tools/conv_isa_table.py --compare parent.csv new.csv > profiles/conv_index_static.md

Compiles gemm2_tiles_*.hip of a csrc/ directory to gfx950 assembly (device only, the build's flags) and reads, for every
instance with a conv operand mode (AM = conv fwd / dgrad gather, BMODE = conv wgrad gather / stored-weight read):
  * NumVgprs, NumAgprs, ScratchSize and Occupancy from the resource-usage block the compiler prints after each kernel
    (the figures of -Rpass-analysis=kernel-resource-usage);
  * the K loop = the largest backward-branch region that holds MFMAs and the K-step's barrier (where the
    compiler lays other blocks inside that span they are counted too, on both sides alike): its MFMA count, its VALU count (v_* without the
    MFMAs), its integer-division sequences (each expands around one v_rcp_iflag_f32) and its v_mul_hi_u32 count (the
    stride's reciprocal multiply).
No GPU needed."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import csv
import re
import subprocess
import sys
import tempfile
from pathlib import Path

MODES = {0: "K", 1: "MN", 2: "conv_fwd", 3: "conv_dgrad", 4: "conv_wgrad", 5: "conv_wt"}
FIELDS = ["instance", "vgprs", "agprs", "scratch", "occupancy", "loop_mfma", "loop_valu", "loop_div", "loop_mulhi"]


def instance_name(sym: str) -> str | None:
    m = re.match(r"_Z12gemm2_kernelI((?:L[ib]\d+E)+)E", sym)
    if not m:
        return None
    v = [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))]
    am, bm, BM, BN, NW, seg2, NS, cs, ldr, npart = v
    if am not in (2, 3) and bm not in (4, 5):
        return None
    name = f"{MODES[am]}|{MODES[bm]} {BM}x{BN} w{NW}"
    for flag, tag in ((seg2, "seg2"), (NS != 2, f"ns{NS}"), (cs, "colsum"), (ldr, f"lora{ldr}")):
        if flag:
            name += " " + tag
    return name


def loop_stats(body: list[str]) -> dict:
    pos = {m.group(1): i for i, ln in enumerate(body) if (m := re.match(r"(\.LBB\d+_\d+):", ln))}
    best = None
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if m and pos.get(m.group(1), i + 1) < i:
            region = body[pos[m.group(1)]:i + 1]
            if any("v_mfma" in r for r in region) and any("s_barrier" in r for r in region) and \
                    (best is None or len(region) > len(best)):
                best = region
    ops =[r.split()[0] for r in (best or []) if re.match(r"\s+[a-z]", r)]
    return {"loop_mfma": sum(o.startswith("v_mfma") for o in ops),
            "loop_valu": sum(o.startswith("v_") and not o.startswith("v_mfma") for o in ops),
            "loop_div": sum(o.startswith("v_rcp_iflag") for o in ops),
            "loop_mulhi": sum(o.startswith("v_mul_hi_u32") for o in ops)}


def parse(asm: str) -> list[dict]:
    rows = []
    for m in re.finditer(r"^(_Z12gemm2_kernel\w+):[^\n]*\n(.*?^; Occupancy: \d+)", asm, re.S | re.M):
        name = instance_name(m.group(1))
        if name is None:
            continue
        text = m.group(2)
        res = {k: int(re.search(rf"; {k}: (\d+)", text).group(1)) for k in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")}
        rows.append({"instance": name, "vgprs": res["NumVgprs"], "agprs": res["NumAgprs"], "scratch": res["ScratchSize"],
                     "occupancy": res["Occupancy"], **loop_stats(text.split("\n"))})
    return rows


def build_table(csrc: Path) -> list[dict]:
    srcs = sorted(csrc.glob("gemm2_tiles_*.hip"))
    with tempfile.TemporaryDirectory() as tmp:
        def one(src: Path) -> str:
            out = Path(tmp) / (src.stem + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                            "--offload-device-only", "-S", "-I", str(csrc), str(src), "-o", str(out)], check=True)
            return out.read_text()
        with cf.ThreadPoolExecutor(len(srcs)) as ex:
            rows = [r for asm in ex.map(one, srcs) for r in parse(asm)]
    return sorted(rows, key=lambda r: r["instance"])


def compare(a_path: str, b_path: str) -> int:
    a = {r["instance"]: r for r in csv.DictReader(open(a_path))}
    b = {r["instance"]: r for r in csv.DictReader(open(b_path))}
    print("| instance (A|B mode, tile, waves) | VGPR+AGPR | scratch B | occupancy | loop MFMA | loop VALU | loop div | loop mul_hi |")
    print("|---|---|---|---|---|---|---|---|")
    bad = 0
    for k in sorted(a):
        x, y = a[k], b[k]
        cell = lambda f: f"{x[f]} -> {y[f]}"
        regs = f"{int(x['vgprs']) + int(x['agprs'])} -> {int(y['vgprs']) + int(y['agprs'])}"
        print(f"| {k} | {regs} | {cell('scratch')} | {cell('occupancy')} | {cell('loop_mfma')} | {cell('loop_valu')} | "
              f"{cell('loop_div')} | {cell('loop_mulhi')} |")
        bad += int(y["scratch"]) > int(x["scratch"]) or int(y["occupancy"]) < int(x["occupancy"]) or int(y["loop_div"]) > 0
    tot = lambda t, f: sum(int(r[f]) for r in t.values())
    print(f"\n{len(a)} instances; K-loop VALU in total {tot(a, 'loop_valu')} -> {tot(b, 'loop_valu')}, division sequences "
          f"{tot(a, 'loop_div')} -> {tot(b, 'loop_div')}; instances that gain scratch, lose occupancy or keep a division: {bad}")
    return 1 if bad or set(a) != set(b) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", type=Path)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_CSV", "NEW_CSV"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    rows = build_table(args.csrc)
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, FIELDS)
        w.writeheader()
        w.writerows(rows)
    print(f"{len(rows)} conv instances -> {args.out}")
