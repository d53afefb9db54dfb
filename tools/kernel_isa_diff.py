#!/usr/bin/env python3
"""Did a source change alter the kernels' code?  usage: kernel_isa_diff.py [--sources=a.hip,b.hip] TREE_A TREE_B [KEEP_DIR]

Compiles csrc/sz_nn.hip and csrc/sz_nn_split.hip (the network kernels; --sources=sz_engine.hip: the tree kernels) of two checkouts for the device only (each tree's own build.py FLAGS plus
--cuda-device-only -S; no GPU needed) and prints one line per kernel: SAME when the instruction text, the .amdhsa_kernel descriptor and the register figures are
identical after stripping comments and numbering the .L labels by first appearance, else DIFF, with both trees' register, scratch and LDS
figures (ONLY-A / ONLY-B: the kernel exists in one tree).  Kernels are matched by demangled name without the parameter list.
KEEP_DIR keeps the .s files."""
import os
import re
import runpy
import shutil
import subprocess
import sys
import tempfile

SOURCES = ["sz_nn.hip", "sz_nn_split.hip"]
FIGURES = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy"]


def compile_s(tree, src, out):
    pkg = os.path.join(tree, "sigma-zero_amd")
    flags = runpy.run_path(os.path.join(pkg, "build.py"))["FLAGS"]
    subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", os.path.join(pkg, "csrc", src), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def short_name(mangled, filt):
    d = subprocess.run([filt, mangled], capture_output=True, text=True).stdout.strip() if filt else mangled
    depth = 0
    for k, ch in enumerate(d):                       # cut the parameter list: the first '(' outside <...>
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            d = d[:k]
            break
    return d[5:] if d.startswith("void ") else d


def kernels(lines, filt):
    """{short name: (normalised text, {figure: value})} of every kernel in an assembly listing"""
    out = {}
    for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines):
        if not m:
            continue
        name = m.group(1)
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        z = next(i for i in range(a, len(lines)) if lines[i].startswith("; Kernel info"))                   # body, descriptor, .set figures, then the info comments
        z = next(i for i in range(z, len(lines)) if lines[i].lstrip().startswith((".text", ".section")) or i == len(lines) - 1)
        labels, text, fig = {}, [], {}
        for l in lines[a:z]:
            f = re.match(r";\s*(\w+):\s*(\d+)", l)
            if f and f.group(1) in FIGURES:
                fig[f.group(1)] = int(f.group(2))
            l = l.split(";")[0].strip().replace(name, "K")
            if l and not l.startswith((".section", ".text", ".p2align", ".protected", ".globl", ".type", ".size")):
                text.append(re.sub(r"\.L\w+", lambda g: ".L%d" % labels.setdefault(g.group(0), len(labels)), l))
        out[short_name(name, filt)] = ("\n".join(text), fig)
    return out


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--sources=")]
    sources = [a[len("--sources="):].split(",") for a in sys.argv[1:] if a.startswith("--sources=")]
    tree_a, tree_b = argv[0], argv[1]
    keep = argv[2] if len(argv) > 2 else None
    work = keep or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")          # without one, kernels are matched by mangled name
    n_diff = 0
    for src in (sources[-1] if sources else SOURCES):
        ka, kb = (kernels(compile_s(t, src, os.path.join(work, "%s_%s.s" % (tag, src))), filt) for tag, t in (("a", tree_a), ("b", tree_b)))
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                print("%-6s %-16s %s" % ("ONLY-A" if k in ka else "ONLY-B", src, k))
            elif ka[k][0] == kb[k][0]:
                print("%-6s %-16s %s" % ("SAME", src, k))
            else:
                n_diff += 1
                print("%-6s %-16s %s   %s" % ("DIFF", src, k, "  ".join("%s %s -> %s" % (f, ka[k][1].get(f), kb[k][1].get(f)) for f in FIGURES)))
    if not keep:
        shutil.rmtree(work)
    print("%d kernel(s) differ" % n_diff)


if __name__ == "__main__":
    main()
