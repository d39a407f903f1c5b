#!/usr/bin/env python3
"""Compiler resource report for the sandwich-norm and GeGLU kernels, bf16 and fp16 objects, against a parent revision
(cross-compiles; no GPU needed).

    python scripts/sandwich_resources.py --parent HEAD~1 > profiles/sandwich_norm_resources.txt

Per kernel: VGPRs, AGPRs, scratch bytes per lane, SGPRs, occupancy, static LDS (hipcc -O3 --offload-arch=gfx950
-munsafe-fp-atomics -Rpass-analysis=kernel-resource-usage, the flags of csrc/build.py) and the code size (the kernel
symbol's size in the device code object, llvm-readelf -s).  Only this metadata of the compiled objects is read.

* csrc/norm.hip and csrc/elementwise.hip: every kernel of the parent beside this tree's ("unchanged" or the
  differing figures).  The three gated-FFN kernels became templates on the activation: the parent's
  ``swiglu_*_kernel`` stands beside this tree's ``swiglu_*_kernel<false>`` (``ILb0E``, the SiLU instantiation).
* the kernels this tree adds: the ``<true>`` (``ILb1E``, GeGLU) instantiations beside their SiLU twins, and every
  kernel of csrc/sandwich_norm.hip.  Names are the mangled ones without the namespace prefix.

* ``sandwich_bwd_kernel<6>`` and ``<8>``, which the extension does not contain, for the record of the fused
  backward's width limit.

Exit status 1 when an existing kernel differs in any figure or a kernel the extension adds uses scratch.
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
HEAD = "kernel\tVGPRs\tAGPRs\tscratch B/lane\tSGPRs\toccupancy waves/SIMD\tstatic LDS B/block\tcode B"


def _build_py():
    spec = importlib.util.spec_from_file_location("dltb_build", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def resources(src, gen, fmt, work, defines=()):
    """{kernel: [VGPRs, AGPRs, scratch, SGPRs, occupancy, LDS, code bytes]} of one compile of ``src``."""
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    readelf = os.path.join(ROCM, "llvm", "bin", "llvm-readelf")
    out = os.path.join(work, f"res_{fmt}.co")
    extra = ["-DDLTB_F16=1", "-include", os.path.join(gen, "fmt_f16_rename.h")] if fmt == "fp16" else []
    cmd = [hipcc, "--offload-device-only", "--no-gpu-bundle-output", "-c", "-fPIC", "-std=c++17",
           "--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics", *extra, *[f"-D{d}" for d in defines], "-I", CSRC,
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
    return {short(k): [v[f] for f in FIELDS] + [sizes[k]] for k, v in res.items()}


def short(name):
    """The mangled kernel name without the anonymous namespace's prefix: name, template arguments (ILb0E... = <false>,
    ILi4ELb1E = <4, true>), parameter types."""
    return re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", name)


def silu_twin(name):
    """(the parent's name of the same kernel without its template argument, is it the GeGLU instantiation) of one of
    the three gated-FFN kernels, else None.  A template instantiation's mangled name also encodes its return type, and
    the template's own name is one more substitution candidate, so the parameter list's S<n>_ back references are
    one higher than the parent's."""
    m = re.match(r"(swiglu_(?:fwd|bwd|bwd_h)_kernel)ILb([01])EEEv(.*)$", name)
    if not m:
        return None
    params = re.sub(r"S(\d)_", lambda s: f"S{int(s.group(1)) - 1}_" if s.group(1) != "0" else "S_", m.group(3))
    return m.group(1) + "E" + params, m.group(2) == "1"


def parent_source(rev, name, work):
    path = os.path.join(work, "parent_" + name)
    with open(path, "w") as f:
        f.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:csrc/{name}"], stdout=subprocess.PIPE, text=True,
                               check=True).stdout)
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="HEAD", help="git revision that holds the parent's kernels (default HEAD)")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as work:
        gen = os.path.join(work, "gen")
        _build_py().gen_format_headers(gen)
        for fmt in ("bf16", "fp16"):
            added = {}
            for name in ("norm.hip", "elementwise.hip"):
                old = resources(parent_source(a.parent, name, work), gen, fmt, work)
                new = resources(os.path.join(CSRC, name), gen, fmt, work)
                renamed = {}
                for k, v in new.items():
                    tw = silu_twin(k)
                    renamed[tw[0] if tw and not tw[1] else k] = v
                print(f"## {fmt} build, csrc/{name}: existing kernels, parent -> this tree")
                print("# " + HEAD + "\tparent -> this tree")
                for k, v in old.items():
                    same = renamed.get(k) == v
                    bad += not same
                    print(k + "\t" + "\t".join(map(str, v)) + "\t" + ("unchanged" if same else f"CHANGED {renamed.get(k)}"))
                added.update({k: (v, old.get(silu_twin(k)[0])) for k, v in renamed.items()
                              if k not in old and silu_twin(k)})
            print(f"## {fmt} build: the GeGLU instantiations, each beside its SiLU twin")
            print("# " + HEAD + "\ttwin: VGPRs / scratch / code B")
            for k, (v, tv) in added.items():
                print(k + "\t" + "\t".join(map(str, v)) + "\t" + (f"{tv[0]} / {tv[2]} / {tv[6]}" if tv else "-"))
                bad += v[2] != 0
            print(f"## {fmt} build, csrc/sandwich_norm.hip: sandwich_fwd_kernel<NV, NEXT>, sandwich_bwd_kernel<NV> (the "
                  "backward's fold image is dynamic LDS: 32 d bytes)")
            print("# " + HEAD)
            built = resources(os.path.join(CSRC, "sandwich_norm.hip"), gen, fmt, work)
            for k, v in built.items():
                print(k + "\t" + "\t".join(map(str, v)))
                bad += v[2] != 0
            print(f"## {fmt} build: sandwich_bwd_kernel<6> and <8>, NOT part of the extension (-DDLTB_SANDWICH_BWD_WIDE): "
                  "why the fused backward stops at 4 register slices, d <= 2048")
            print("# " + HEAD)
            wide = resources(os.path.join(CSRC, "sandwich_norm.hip"), gen, fmt, work, ["DLTB_SANDWICH_BWD_WIDE=1"])
            for k, v in wide.items():
                if k not in built:
                    print(k + "\t" + "\t".join(map(str, v)))
    if bad:
        print(f"# {bad} kernel(s) changed or use scratch")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
