#!/usr/bin/env python3
"""Per-kernel comparison of the generated gfx950 assembly of two trees (docs/EXPERIMENTS.md R7.1): for a refactor of the tile engines.

    python tools/isa_diff.py OLD [NEW] [--files gcn_tile linear conv stem] [--markdown]

OLD / NEW: a git revision (exported with `git archive`) or a directory holding a tree; NEW defaults to the working tree.  Every file is compiled
device-only with the library's flags (egohmr_amd/_lib.py), lines naming the compiler or the compilation unit's id are dropped, and the text is cut
at the kernels' mangled-name labels.  Class A = the kernel's text is identical; B = it differs, and the resource figures of the code object's
metadata and the static counts of the instructions that shape the K loop are printed, OLD -> NEW.  Needs no GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
COUNTS = {"mfma": r"^\s*v_mfma_", "ds_read_b128": r"^\s*ds_read_b128", "dma": r"^\s*buffer_load_dword.*\blds\b", "barrier": r"^\s*s_barrier",
          "vmcnt": r"^\s*s_waitcnt.*vmcnt", "setprio": r"^\s*s_setprio"}


def tree_of(spec, tmp):
    if os.path.isdir(spec):
        return os.path.abspath(spec)
    out = os.path.join(tmp, "tree_" + re.sub(r"\W", "_", spec))
    os.makedirs(out)
    tar = subprocess.run(["git", "-C", ROOT, "archive", spec, "egohmr_amd/csrc", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", out], input=tar, check=True)
    return out


def kernels_of(tree, name, tmp):
    """{mangled kernel name: (text, {metadata key: int})} of csrc/<name>.hip"""
    out = os.path.join(tmp, f"{abs(hash(tree))}_{name}.s")
    csrc, inc = os.path.join(tree, "egohmr_amd", "csrc"), os.path.join(tree, "include")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{inc}", f"-I{csrc}",
                    "--offload-device-only", "-S", os.path.join(csrc, name + ".hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
    lines = [l for l in open(out).read().split("\n") if ".ident" not in l and "__hip_cuid" not in l]
    body, _, meta = "\n".join(lines).partition(".amdgpu_metadata")
    text, cur = {}, None
    for l in body.split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        cur = m.group(1) if m else cur
        if cur:
            text.setdefault(cur, []).append(l)
    res = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        kname = re.search(r"\.name:\s+(\S+)", entry).group(1)
        res[kname] = ("\n".join(text[kname]), {k: int(re.search(re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in META})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=ROOT)
    ap.add_argument("--files", nargs="+", default=["gcn_tile", "linear", "conv", "stem"])
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as ex:
        trees = [tree_of(a.old, tmp), tree_of(a.new, tmp)]
        jobs = {(t, f): ex.submit(kernels_of, t, f, tmp) for t in trees for f in a.files}

        def demangle(n):
            try:
                return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "").split("(")[0] or n
            except OSError:
                return n
        differing = 0
        for f in a.files:
            old, new = jobs[(trees[0], f)].result(), jobs[(trees[1], f)].result()
            for k in sorted(set(old) | set(new)):
                if k not in old or k not in new:
                    cls, detail = "-", "only in " + ("OLD" if k in old else "NEW")
                elif old[k][0] == new[k][0]:
                    cls, detail = "A", ""
                else:
                    cls = "B"
                    m = [f"{key[1:]} {old[k][1][key]} -> {new[k][1][key]}" for key in META]
                    c = [f"{key} {n0} -> {n1}" for key, rx in COUNTS.items()
                         for n0, n1 in [[len(re.findall(rx, t[k][0], re.M)) for t in (old, new)]]]
                    detail = "; ".join(m + c)
                differing += cls != "A"
                print(f"| {f}.hip | `{demangle(k)}` | {cls} | {detail} |" if a.markdown else f"{cls}  {f}.hip  {demangle(k)}  {detail}")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
