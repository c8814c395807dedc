#!/usr/bin/env python3
"""Diff the gfx950 machine code of the tg_demo_items kernels between two builds of mat_mul_amd/csrc/tg_items.hip.

    hipcc <build.FLAGS> -c mat_mul_amd/csrc/tg_items.hip -o new.o      (and the same at the other revision: old.o)
    python tools/items_disasm_diff.py old.o new.o

Extracts the gfx950 code object from each host object's .hip_fatbin (llvm-objcopy, clang-offload-bundler), disassembles
every items_* kernel symbol (llvm-objdump -d, raw bytes kept, addresses dropped; c++filt demangles) and diffs them
kernel by kernel.  The kernels became templates over a row-resolution policy (tg_items.h), so a kernel is matched by its demangled name with
the policy argument ``tg::DemoRows`` and the empty argument pack removed; the symbol names inside the listings are
replaced by that key.  Prints the diff (empty when identical) and exits 1 when any kernel differs or is missing."""
from __future__ import annotations

import difflib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _run(*cmd) -> str:
    return subprocess.run([str(c) for c in cmd], check=True, capture_output=True, text=True).stdout


def key(sym: str) -> str:
    name = _run("c++filt", sym).strip()
    name = name.replace("tg::DemoRows, ", "").replace(", tg::ItemArgs)", ")")
    return re.sub(r"\(tg::ItemArgs(, )?\)", "(tg::ItemArgs)", name)


def listings(obj: Path, tmp: Path) -> dict:
    fat, co = tmp / f"{obj.stem}.fatbin", tmp / f"{obj.stem}.co"
    _run(LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, tmp / "discard.o")
    _run(LLVM / "clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}",
         f"--output={co}")
    syms = sorted({ln.split()[7] for ln in _run(LLVM / "llvm-readelf", "-sW", co).splitlines()
                   if len(ln.split()) >= 8 and ln.split()[3] == "FUNC" and "items_" in ln.split()[7]})
    out = {}
    for s in syms:
        text = _run(LLVM / "llvm-objdump", "-d", "--no-leading-addr", f"--disassemble-symbols={s}", co)
        body = text[text.index(f"<{s}>:"):]
        body = re.sub(r"// [0-9A-F]+:", "//", body)          # the address column of the raw bytes
        body = re.sub(r"// [0-9A-F]+ <", "// <", body)       # branch targets: keep the symbol-relative form
        k = key(s)
        out[k] = body.replace(s, k).splitlines()
    return out


def main(old: str, new: str) -> int:
    with tempfile.TemporaryDirectory() as d:
        for sub in ("a", "b"):
            (Path(d) / sub).mkdir()
        a = listings(Path(old), Path(d) / "a")
        b = listings(Path(new), Path(d) / "b")
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"only in {'new' if k in b else 'old'}: {k}")
            bad += k in a  # new kernels (other policies) are expected; a lost one is not
            continue
        diff = list(difflib.unified_diff(a[k], b[k], f"old {k}", f"new {k}", lineterm=""))
        if diff:
            bad += 1
            print("\n".join(diff))
    print(f"{len(set(a) & set(b))} kernels compared, {bad} differ or are missing", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
