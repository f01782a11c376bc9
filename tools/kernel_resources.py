"""Register / scratch / spill / occupancy table of the kernels of some csrc/*.hip files, from the compiler's
kernel-resource remarks (-Rpass-analysis=kernel-resource-usage; cross-compiles without a GPU).

    python tools/kernel_resources.py scan_fwd scan_seg dwconv > now.json
    python tools/kernel_resources.py --diff before.json now.json          # markdown table, changed rows marked

Used to show that a change to a kernel's source left the shipped instantiations where they were (no new spills, no
kernel across an occupancy step): run it on the parent commit and on the change."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cleanumamba_amd", "csrc")
FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch",
          "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill", "Occupancy [waves/SIMD]": "occupancy",
          "LDS Size [bytes/block]": "lds"}


def remarks(name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-Wno-unused-value",
           "-Rpass-analysis=kernel-resource-usage", "-c", name + ".hip", "-o", os.devnull]
    return subprocess.run(cmd, cwd=CSRC, check=True, capture_output=True, text=True).stderr


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return out.stdout.split("\n") if out.returncode == 0 else names


def short(name):
    """`void cum::k<3, float, false>(cum::ScanParams)` -> `k<3, float>`: a trailing `false` template argument (a
    feature switch that is off, e.g. ENTER) is dropped, so the row lines up with a parent that lacks the parameter."""
    if name.startswith("_Z"):           # (binutils' c++filt does not know _Float16 / __bf16: the name stays mangled)
        return re.sub(r"Lb0E(E+v)", r"\1", name)
    name = re.sub(r"^void ", "", name.replace("cum::", ""))
    name = re.sub(r"\((ScanParams|ConvParams)[^)]*\)$", "", name)
    return re.sub(r", false>$", ">", name)


def parse(text):
    table, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = table.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val) if val.isdigit() else val
    names = list(table)
    return {short(d): table[n] for n, d in zip(names, demangle(names))}


def diff(a, b):
    cols = ["vgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy"]
    print("| kernel | " + " | ".join(f"{c} before -> after" for c in cols) + " |")
    print("|---|" + "---|" * len(cols))
    changed = 0
    for k in sorted(set(a) | set(b)):
        ra, rb = a.get(k), b.get(k)
        cells = [f"{'-' if ra is None else ra.get(c)} -> {'-' if rb is None else rb.get(c)}" for c in cols]
        mark = "" if ra is not None and rb is not None and all(ra.get(c) == rb.get(c) for c in cols) else " **"
        changed += bool(mark)
        print(f"| `{k}`{mark} | " + " | ".join(cells) + " |")
    print(f"\n{len(set(a) | set(b))} kernels, {changed} with a changed or new row (marked **).")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--diff"]:
        diff(json.load(open(sys.argv[2])), json.load(open(sys.argv[3])))
    else:
        res = {}
        for f in sys.argv[1:] or ["scan_fwd", "scan_seg"]:
            res.update(parse(remarks(f)))
        json.dump(res, sys.stdout, indent=1, sort_keys=True)
