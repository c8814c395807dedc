#!/usr/bin/env python3
"""Diff the gfx950 machine code and kernel metadata of two builds of the library, object by object.

    python -m mat_mul_amd.build --force          (and/or --ab; the same in the other checkout)
    python tools/disasm_diff.py <old>/mat_mul_amd/lib/obj <new>/mat_mul_amd/lib/obj

For every host object (``*.o``) of the two directories it extracts the gfx950 code object from the ``.hip_fatbin``
section (llvm-objcopy, clang-offload-bundler), disassembles it once (llvm-objdump -d, raw bytes kept, addresses and the
padding between functions dropped) and diffs every function symbol's listing, matched by symbol.  It also diffs each
kernel's AMDHSA metadata (llvm-readelf --notes: VGPR/SGPR counts, LDS and scratch sizes, arguments), matched by
``.name``.  Prints the differences and the objects or kernels present on one side only, and exits 1 on any of them,
0 when the two builds are identical."""
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


def code_object(obj: Path, tmp: Path) -> Path:
    fat, co = tmp / f"{obj.name}.fatbin", tmp / f"{obj.name}.co"
    _run(LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, tmp / "discard.o")
    _run(LLVM / "clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}",
         f"--output={co}")
    return co


def listings(co: Path) -> dict:
    """symbol -> its disassembly, without the address column (branch targets stay in their symbol-relative form)"""
    out, cur = {}, None
    for ln in _run(LLVM / "llvm-objdump", "-d", "--no-leading-addr", co).splitlines():
        m = re.fullmatch(r"<(.+)>:", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip() not in ("", "..."):  # ("...": the padding after a function)
            cur.append(re.sub(r"// [0-9A-F]+:", "//", re.sub(r"// [0-9A-F]+ <", "// <", ln)))
    return out


def metadata(co: Path) -> dict:
    """kernel name -> its block of the AMDGPU metadata note (YAML lines)"""
    out, block = {}, None
    for ln in _run(LLVM / "llvm-readelf", "--notes", co).splitlines():
        if ln.startswith("  - ."):  # a new entry of amdhsa.kernels
            block = [ln]
        elif block is not None and ln.startswith("    "):
            block.append(ln)
            m = re.match(r"\s{4}\.name:\s+(\S+)", ln)
            if m:
                out[m.group(1)] = block
        else:
            block = None
    return out


def diff_maps(what: str, a: dict, b: dict) -> int:
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{what}: only in {'new' if k in b else 'old'}: {k}")
            bad += 1
            continue
        d = list(difflib.unified_diff(a[k], b[k], f"old {k}", f"new {k}", lineterm=""))
        if d:
            print(f"{what}:")
            print("\n".join(d))
            bad += 1
    return bad


def main(old: str, new: str) -> int:
    objs = {p.name for p in Path(old).glob("*.o")} | {p.name for p in Path(new).glob("*.o")}
    bad = kernels = 0
    with tempfile.TemporaryDirectory() as d:
        for name in sorted(objs):
            sides = [Path(old) / name, Path(new) / name]
            if not all(p.exists() for p in sides):
                print(f"{name}: only in {'new' if sides[1].exists() else 'old'}")
                bad += 1
                continue
            cos = []
            for tag, p in zip("ab", sides):
                (Path(d) / tag).mkdir(exist_ok=True)
                cos.append(code_object(p, Path(d) / tag))
            code = [listings(c) for c in cos]
            meta = [metadata(c) for c in cos]
            n_bad = diff_maps(f"{name} code", *code) + diff_maps(f"{name} metadata", *meta)
            kernels += len(set(meta[0]) & set(meta[1]))
            print(f"{name}: {len(set(code[0]) & set(code[1]))} symbols, {len(set(meta[0]) & set(meta[1]))} kernels compared, "
                  f"{n_bad} differ or are missing", file=sys.stderr)
            bad += n_bad
    print(f"{len(objs)} objects, {kernels} kernels compared, {bad} differences", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
