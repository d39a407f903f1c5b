#!/usr/bin/env python3
"""Compiler resource report of every kernel of csrc/xent.hip, bf16 and fp16 objects, for a parent revision and for this
tree (cross-compiles; no GPU needed).

    python scripts/xent_resources.py --parent HEAD > profiles/xent_resources.txt

Per kernel: VGPRs, AGPRs, scratch bytes per lane, SGPRs, occupancy, static LDS (hipcc -O3 --offload-arch=gfx950
-munsafe-fp-atomics -Rpass-analysis=kernel-resource-usage, the flags of csrc/build.py) and the code size (the kernel
symbol's size in the device code object, llvm-readelf -s).  The first table per format lists the parent's kernels
beside this tree's ("unchanged" or the differing figures); the second the kernels this tree adds, each option kernel
beside its plain twin.  Exit status 1 when an existing kernel differs or an option kernel with VPT <= 8 uses scratch.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FIELDS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "TotalSGPRs", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]"]


def _build_py():
    spec = importlib.util.spec_from_file_location("dltb_build", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def resources(src, gen, fmt, work):
    """{kernel: [VGPRs, AGPRs, scratch, SGPRs, occupancy, LDS, code bytes]} of one compile of ``src``."""
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    readelf = os.path.join(ROCM, "llvm", "bin", "llvm-readelf")
    out = os.path.join(work, f"xent_{fmt}.co")
    extra = ["-DDLTB_F16=1", "-include", os.path.join(gen, "fmt_f16_rename.h")] if fmt == "fp16" else []
    cmd = [hipcc, "--offload-device-only", "--no-gpu-bundle-output", "-c", "-fPIC", "-std=c++17",
           "--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics", *extra, "-I", CSRC,
           "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout)
    res, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    sizes = {}
    for line in subprocess.run([readelf, "-sW", out], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            sizes[p[7]] = int(p[2])
    return {k: [v[f] for f in FIELDS] + [sizes[k]] for k, v in res.items()}


def short(name):
    return re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", name)


def twin(name):
    """The plain kernel an option kernel stands beside: same VPT, without the CAP argument and the _opt in its name."""
    m = re.match(r"(xent(?:_lse|_bwd_lse)?)_opt_kernelIL?i?(\d*)E?Lb[01]E", short(name))
    if not m:
        return None
    return m.group(1) + "_kernel", m.group(2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="HEAD", help="git revision whose csrc/xent.hip is the parent (default HEAD)")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as work:
        gen = os.path.join(work, "gen")
        _build_py().gen_format_headers(gen)
        parent_src = os.path.join(work, "xent_parent.hip")
        with open(parent_src, "w") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{a.parent}:csrc/xent.hip"], stdout=subprocess.PIPE,
                                   text=True, check=True).stdout)
        head = "kernel\tVGPRs\tAGPRs\tscratch B/lane\tSGPRs\toccupancy waves/SIMD\tstatic LDS B/block\tcode B"
        for fmt in ("bf16", "fp16"):
            old = resources(parent_src, gen, fmt, work)
            new = resources(os.path.join(CSRC, "xent.hip"), gen, fmt, work)
            print(f"## {fmt} build: existing kernels, parent -> this tree")
            print("# " + head + "\tparent -> this tree")
            for k, v in old.items():
                same = new.get(k) == v
                bad += not same
                print(short(k) + "\t" + "\t".join(map(str, v)) + "\t" + ("unchanged" if same else f"CHANGED {new.get(k)}"))
            print(f"## {fmt} build: the option kernels <VPT, CAP> (CAP = Lb1: the capped instantiation), each beside "
                  "its plain twin")
            print("# " + head + "\ttwin: VGPRs / scratch / code B")
            by_short = {short(k): v for k, v in old.items()}
            for k, v in new.items():
                if k in old:
                    continue
                base, vpt = twin(k)
                tname = next((s for s in by_short if s.startswith(base + (f"ILi{vpt}E" if vpt else "E"))), None)
                tv = by_short.get(tname)
                print(short(k) + "\t" + "\t".join(map(str, v)) + "\t"
                      + (f"{tv[0]} / {tv[2]} / {tv[6]}" if tv else "-"))
                if vpt and int(vpt) <= 8 and "Lb1E" in short(k) and v[2] != 0:
                    bad += 1
                    print(f"# SCRATCH in a capped VPT <= 8 instantiation: {short(k)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
