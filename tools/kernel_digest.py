#!/usr/bin/env python3
"""One line per kernel of a HIP source: what the compiler made of it.

  tools/kernel_digest.py binary-image-compression_amd/csrc/bic_fused.hip [more.hip ...] [-D...] [-o FILE]

Compiles each source for the device alone (gfx950) and prints, sorted, per kernel:
  demangled name | vgpr_count sgpr_count private_segment_fixed_size group_segment_fixed_size | sha256
the counts from the code object's notes, the hash over the kernel's instruction bytes (its FUNC
symbol's address and size). Two builds whose lines are equal give the GPU the same kernels; a refactor
of the host side, or a move of kernels between sources, must leave the lines as they were
(profiles/r09/kernels_*.txt). No GPU is needed.
"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "binary-image-compression_amd")
LLVM = os.environ.get("BIC_LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def digest(src, defines, arch):
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "k.o")
        run(HIPCC, f"--offload-arch={arch}", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(PKG, "csrc"), *defines, "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", obj,
            src)
        readelf = os.path.join(LLVM, "llvm-readelf")
        # the notes: under amdhsa.kernels one block per kernel, begun by "  - .key: value", its own
        # keys indented by four spaces (deeper ones belong to its arguments)
        notes, cur = {}, None
        for line in run(readelf, "--notes", obj).splitlines():
            m = re.match(r"  (- |  )\.(\w+):\s*(.*)$", line)
            if not m:
                continue
            if m.group(1) == "- ":
                cur = {}
            if cur is None:
                continue
            key, val = m.group(2), m.group(3).strip().strip("'")
            if key == "symbol":
                notes[val[:-3] if val.endswith(".kd") else val] = cur
            elif key in FIELDS:
                cur[key] = val
        # sections and symbols
        text = None
        for line in run(readelf, "-S", "--wide", obj).splitlines():
            m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
            if m:
                text = tuple(int(x, 16) for x in m.groups())  # address, file offset, size
        if text is None:
            raise SystemExit(f"{src}: no .text section")
        blob = open(obj, "rb").read()
        funcs = {}
        for line in run(readelf, "-s", "--wide", obj).splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC" and p[7] in notes:
                funcs[p[7]] = (int(p[1], 16), int(p[2]))
        missing = sorted(set(notes) - set(funcs))
        if missing:
            raise SystemExit(f"{src}: kernels without a FUNC symbol: {missing}")
        names = run(shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt"), *sorted(funcs)).splitlines()
        lines = []
        for sym, name in zip(sorted(funcs), names):
            addr, size = funcs[sym]
            off = text[1] + addr - text[0]
            if addr < text[0] or addr + size > text[0] + text[2]:
                raise SystemExit(f"{src}: {sym} lies outside .text")
            h = hashlib.sha256(blob[off:off + size]).hexdigest()
            lines.append(f"{name} | " + " ".join(str(notes[sym].get(f, "?")) for f in FIELDS) + f" | {h}")
        return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="+")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor definitions for the build")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("-o", dest="out", help="write the listing here instead of standard output")
    a = ap.parse_args()
    lines = []
    for src in a.sources:
        lines += digest(src, ["-D" + d for d in a.defines], a.arch)
    text = "".join(l + "\n" for l in sorted(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        print(f"{len(lines)} kernels -> {a.out}", file=sys.stderr)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
