#!/usr/bin/env python3
"""Static spill report of a HIP source's gfx950 kernels (the fused-variant hang).

  python3 tools/spill_check.py [csrc/art_trace.hip] [-DFLAG ...]

(The default source holds the raytrace stage; the permeation kernels are a second source, csrc/art_permeate.hip,
the muffle cell lists and the target syncs' kernels a third, csrc/art_cells.hip: profiles/targets_resize_spill.txt,
the BVH build, refit and relabel kernels a fourth, csrc/art_bvh.hip: profiles/colliders_resize_spill.txt,
the per-sample DSP, the tick, the mix and dsp_sources_follow_kernel a fifth, csrc/art_dsp.hip:
profiles/sources_follow_spill.txt, with dsp_tick_params_classes_kernel profiles/tick_classes_spill.txt.)

For every kernel: its VGPR count, scratch, LDS, occupancy and code length, and for each spill slot the stores and reloads
with the loop they sit in (the compiler's "Loop Header" / "in Loop" block annotations). A spill
stored inside a divergent loop (a narrowed exec mask) and reloaded after it can hand the reloading
lanes values they never stored; spills outside every loop are read back by the lanes that stored them."""
import re
import subprocess
import sys
import tempfile

root = __file__.rsplit("/tools/", 1)[0]
src = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else f"{root}/audio-raytracer_amd/csrc/art_trace.hip"
flags = [a for a in sys.argv[1:] if a.startswith("-")]
import os
src = os.path.abspath(src)
with tempfile.TemporaryDirectory() as d:
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--save-temps", *flags, "-c",
                    src, "-o", f"{d}/o.o"], cwd=d, check=True, capture_output=True)
    import glob
    asm = open(glob.glob(f"{d}/*gfx950.s")[0]).read().splitlines()

kernels, cur, last = [], None, None
for i, line in enumerate(asm):
    m = re.match(r"^(_Z\S+):\s*;\s*@", line)
    if m:
        cur = last = {"name": m.group(1), "lines": [], "res": {}}
        kernels.append(cur)
        continue
    if cur is not None:
        if line.startswith(".Lfunc_end"):
            cur = None
        else:
            cur["lines"].append(line)
    elif last is not None:  # the resource comments that follow a kernel's code
        m = re.match(r"^; (NumVgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", line) or re.match(r"^; (codeLenInByte) = (\d+)", line)
        if m:
            last["res"].setdefault(m.group(1), int(m.group(2)))

def demangle(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "").split("(")[0]

for k in kernels:
    loop = "not in a loop"
    sites = []
    for line in k["lines"]:
        if re.match(r"^(\.LBB\S+:|; %bb\.\d+:)", line):  # a block label: its loop annotation, if any
            loop = line.split(";", 1)[1].strip() if ("Loop" in line and ";" in line) else "not in a loop"
        elif "Loop Header" in line or "in Loop" in line or "Parent Loop" in line:
            loop = line.split(";", 1)[1].strip()
        m = re.search(r"scratch_(store|load)_dword\w*\s", line)
        if m:
            off = re.search(r"offset:(\d+)", line)
            sites.append((m.group(1), int(off.group(1)) if off else 0, loop))
    name = demangle(k["name"])
    if k["res"]:  # every kernel: registers, scratch, LDS, occupancy and code length as the compiler reports them
        r = k["res"]
        print(f"{name[:160]}: {r.get('NumVgprs', '?')} VGPRs, scratch {r.get('ScratchSize', '?')} B, "
              f"LDS {r.get('LDSByteSize', '?')} B, occupancy {r.get('Occupancy', '?')}, code {r.get('codeLenInByte', '?')} B")
    if not sites:
        continue
    print(f"{name[:160]}: {len(sites)} scratch ops")
    for kind, off, lp in sites[:int(os.environ.get("SPILL_SITES", "1000"))]:
        print(f"   {kind:5s} slot {off:3d}  {lp}")
print("kernels with scratch:", sum(1 for k in kernels if any("scratch_" in l for l in k["lines"])), "of", len(kernels))
