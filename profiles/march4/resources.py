"""Per-kernel resource lines and instruction counts of translation units, from the compiler alone (no GPU).
Usage: python profiles/march4/resources.py <repository root> <output directory> <unit> [<unit> ...]
  e.g. python profiles/march4/resources.py . profiles/march4/after kernels_stencil4 kernels_stencil44
Each unit csrc/src/<unit>.hip is compiled once with the project's HIP flags (tools/build.py HIP_FLAGS) plus
  --cuda-device-only -Rpass-analysis=kernel-resource-usage -S
and gives <unit>.resources.txt (VGPRs, AGPRs, scratch, occupancy, LDS per kernel) and <unit>.instructions.txt (the
instructions between a kernel's label and its end in the -S output), both keyed by the demangled kernel name without
its parameter types and sorted by it."""
import os, re, subprocess, sys

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
root, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
os.makedirs(out, exist_ok=True)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", f"-I{root}/csrc/include",
         "--offload-arch=gfx950", "-fno-gpu-rdc", "-munsafe-fp-atomics",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S"]


def names(mangled):
    r = subprocess.run(["c++filt", "-p"], input="\n".join(mangled), capture_output=True, text=True,
                       check=True)
    return dict(zip(mangled, (re.sub(r"^(void )?(wave3d::)?(\(anonymous namespace\)::)?", "", n) for n in r.stdout.splitlines())))


for unit in sys.argv[3:]:
    asm = os.path.join(out, unit + ".s")
    r = subprocess.run([f"{ROCM}/bin/hipcc", *FLAGS, f"{root}/csrc/src/{unit}.hip", "-o", asm], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        else:
            cur[m.group(1).split()[0]] = m.group(2)
    counts, cur = {}, None
    for line in open(asm):
        m = re.match(r"(\w+):", line)
        if m and m.group(1) in res:
            cur = m.group(1)
            counts[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"\t[a-z]\w*( |$)", line):
            counts[cur] += 1
    os.remove(asm)
    nm = names(list(res))
    with open(os.path.join(out, unit + ".resources.txt"), "w") as f:
        for k in sorted(res, key=nm.get):
            v = res[k]
            f.write(f"{nm[k]:<64} | VGPR {v['VGPRs']} AGPR {v['AGPRs']} scratch {v['ScratchSize']} occ {v['Occupancy']} "
                    f"LDS {v['LDS']}\n")
    with open(os.path.join(out, unit + ".instructions.txt"), "w") as f:
        for k in sorted(counts, key=nm.get):
            f.write(f"{nm[k]:<64} | {counts[k]}\n")
    print(unit, len(res), "kernels")
