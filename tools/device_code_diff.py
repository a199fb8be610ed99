#!/usr/bin/env python
"""Compare the gfx950 device code of two source trees, file by file.

    python tools/device_code_diff.py OLD_TREE NEW_TREE [-j JOBS]

Each tree is a checkout (or a `git archive` export) holding pyabc_amd/ and
include/.  Every .hip file of pyabc_amd/csrc is compiled to device assembly
with the flags of that tree's own pyabc_amd/build.py (FLAGS and EXTRA,
imported) plus --offload-device-only -S.  Per file the tool prints whether
the assembly is identical (the __hip_cuid lines, a hash of the source path,
dropped), and per kernel the figures of the code object metadata: VGPRs,
SGPRs, private (scratch) segment, group (LDS) segment.  Kernels whose figures
or code differ and kernel names present in one tree only are listed.  Needs
hipcc and no GPU.  Exit status 1 when any file differs.
"""
import argparse
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

FIGURES = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"),
           ("private", "private_segment_fixed_size"),
           ("group", "group_segment_fixed_size"))
# kernel-level keys of amdhsa.kernels sit at this indent (argument entries,
# which also have a .name, are nested deeper)
KEY = re.compile(r"^    \.(name|%s):\s+(\S+)\s*$" % "|".join(k for _, k in FIGURES))
FUNC_LABEL = re.compile(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$")   # "name:  ; @name"
LOCAL_LABEL =re.compile(r"\.L(BB|func_end|func_begin|JTI)\d+")


def load_build(tree):
    path = os.path.join(tree, "pyabc_amd", "build.py")
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(tree))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(build, src, out):
    cmd = ([build.HIPCC] + build.FLAGS + build.EXTRA.get(os.path.basename(src), []) +
           ["--offload-device-only", "-S", src, "-o", out])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    with open(out) as f:
        return [ln for ln in f.read().splitlines() if "__hip_cuid" not in ln]


def kernel_figures(lines):
    """{kernel name: {figure: value}} from the .amdgpu_metadata block."""
    kernels, cur = {}, None
    inside = False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and ln.startswith("  - "):       # next kernel entry
            cur = {}
            ln = "    " + ln[4:]
        elif inside and ln and not ln.startswith(" "):
            inside = False
        if not inside or cur is None:
            continue
        m = KEY.match(ln)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                kernels[m.group(2)] = cur
    return {n: {short: int(k[key]) for short, key in FIGURES} for n, k in kernels.items()}


def kernel_bodies(lines, names):
    """{kernel name: its instructions}, local label numbers normalised."""
    bodies, cur = {}, None
    for ln in lines:
        if cur is None:
            m = FUNC_LABEL.match(ln)
            if m and m.group(1) in names:
                cur = m.group(1)
                bodies[cur] = []
        elif ln.startswith(".Lfunc_end"):
            cur = None
        else:
            code = LOCAL_LABEL.sub(r".L\1", ln.split(";")[0].rstrip())   # comments name labels too
            if code:
                bodies[cur].append(code)
    return bodies


def compare_file(name, builds, trees, tmp):
    asm = []
    for side, (build, tree) in enumerate(zip(builds, trees)):
        src = os.path.join(tree, "pyabc_amd", "csrc", name)
        asm.append(device_asm(build, src, os.path.join(tmp, f"{side}_{name}.s"))
                   if os.path.exists(src) else None)
    return name, asm


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--only", action="append", metavar="FILE",
                    help="compare this .hip file only (may be repeated)")
    args = ap.parse_args()
    trees = [os.path.abspath(args.old_tree), os.path.abspath(args.new_tree)]
    builds = [load_build(t) for t in trees]
    names = sorted({f for t in trees for f in os.listdir(os.path.join(t, "pyabc_amd", "csrc"))
                    if f.endswith(".hip") and (not args.only or f in args.only)})
    ndiff = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(args.jobs) as ex:
        results = list(ex.map(lambda n: compare_file(n, builds, trees, tmp), names))
    for name, (old, new) in results:
        if old is None or new is None:
            print(f"== {name}: only in the {'new' if old is None else 'old'} tree")
            ndiff += 1
            continue
        same = old == new
        ndiff += not same
        fo, fn = kernel_figures(old), kernel_figures(new)
        print(f"== {name}: {'identical' if same else 'different'} "
              f"({len(fo)} / {len(fn)} kernels)")
        for k in sorted(set(fo) - set(fn)):
            print(f"   only in the old tree: {k}")
        for k in sorted(set(fn) - set(fo)):
            print(f"   only in the new tree: {k}")
        bo, bn = kernel_bodies(old, set(fo)), kernel_bodies(new, set(fn))
        for k in sorted(set(fo) & set(fn)):
            fig = " ".join(f"{s}={fn[k][s]}" for s, _ in FIGURES)
            if fo[k] != fn[k]:
                was = " ".join(f"{s}={fo[k][s]}" for s, _ in FIGURES)
                print(f"   FIGURES DIFFER {k}: {was} -> {fig}")
            elif bo[k] != bn[k]:
                print(f"   code differs   {k}: {fig} (figures equal)")
            else:
                print(f"   {k}: {fig}")
    print(f"{len(names) - ndiff} of {len(names)} files identical")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
