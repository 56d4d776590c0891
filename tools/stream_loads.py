#!/usr/bin/env python3
"""Which global loads and stores of the BUILT library carry the non-temporal hint (`nt`), per kernel.

    python tools/stream_loads.py [libdsp_amd.so] [substring of the demangled kernel name]

Reads the gfx950 code objects out of the library's .hip_fatbin section (one clang offload bundle per translation unit),
disassembles them with the ROCm llvm-objdump and counts, per kernel symbol and per mnemonic, the global_load_* /
global_store_* instructions with and without the `nt` modifier.  The source only ASKS for the hint
(__builtin_nontemporal_load / _store, csrc/stream_load.hpp); the optimiser is free to lose it (it did: DESIGN.md 3.1),
so the binary is the place to look.  tests/test_stream_loads_cpu.py asserts the per-kernel rules on this module's output.
"""
from __future__ import annotations

import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def find_tool(name: str) -> str | None:
    """The ROCm LLVM tool `name` (llvm-objdump, llvm-objcopy): next to hipcc's clang first, then $PATH."""
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc")
    if hipcc:
        roots.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for r in roots:
        for sub in ("llvm/bin", "lib/llvm/bin"):
            cand = os.path.join(r, sub, name) if r else None
            if cand and os.path.exists(cand):
                return cand
    return shutil.which(name)


def tools_present() -> bool:
    return all(find_tool(t) for t in ("llvm-objdump", "llvm-objcopy")) and shutil.which("c++filt") is not None


def code_objects(lib: str, arch: str = "gfx950") -> list[bytes]:
    """Every device ELF for `arch` in the library's .hip_fatbin (uncompressed clang offload bundles, one per source file)."""
    with tempfile.TemporaryDirectory() as d:
        sec = os.path.join(d, "fatbin")
        subprocess.check_call([find_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={sec}", lib, os.path.join(d, "unused")])
        with open(sec, "rb") as f:
            blob = f.read()
    out = []
    pos = blob.find(BUNDLE_MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(BUNDLE_MAGIC))
        p = pos + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.startswith("hip") and triple.split("-")[-1].split(":")[0] == arch and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(BUNDLE_MAGIC, pos + len(BUNDLE_MAGIC))
    return out


_SYM = re.compile(r"^[0-9a-f]+ <([^>]+)>:\s*$")
_INS = re.compile(r"^\s+(global_(?:load|store)_\w+)\s+([^/]*)")


def disassemble(lib: str) -> dict[str, list[str]]:
    """{demangled kernel or function name: its global_load_* / global_store_* lines, in program order, as
    "<mnemonic> <operands and modifiers>"}."""
    per_sym: dict[str, list[str]] = {}
    objdump = find_tool("llvm-objdump")
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(code_objects(lib)):
            path = os.path.join(d, f"{k}.co")
            with open(path, "wb") as f:
                f.write(co)
            text = subprocess.run([objdump, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                m = _SYM.match(line)
                if m:
                    cur = m.group(1)
                    per_sym.setdefault(cur, [])
                    continue
                m = _INS.match(line)
                if m and cur is not None:
                    per_sym[cur].append(f"{m.group(1)} {m.group(2).strip()}")
    names = list(per_sym)
    dem = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return {d_: per_sym[n] for n, d_ in zip(names, dem)}


def is_nt(ins: str) -> bool:
    return re.search(r"(^|\s)nt(\s|$)", ins) is not None


def count(lines: list[str]) -> dict[str, tuple[int, int]]:
    """{mnemonic: (with nt, without nt)}"""
    res: dict[str, tuple[int, int]] = {}
    for ins in lines:
        mn = ins.split()[0]
        a, b = res.get(mn, (0, 0))
        res[mn] = (a + 1, b) if is_nt(ins) else (a, b + 1)
    return res


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "dsp_amd", "libdsp_amd.so")
    sub = sys.argv[2] if len(sys.argv) > 2 else ""
    total = 0
    for name, lines in sorted(disassemble(lib).items()):
        c = count(lines)
        total += sum(a for a, _ in c.values())
        if sub in name and any(a for a, _ in c.values()) or (sub and sub in name):
            short = re.sub(r"\((?!anonymous namespace\)).*", "", name)
            print(f"{short[:120]:120s} " + "  ".join(f"{mn.replace('global_', '')} nt {a} plain {b}" for mn, (a, b) in sorted(c.items())))
    print(f"# {total} non-temporal global loads and stores in {lib}")


if __name__ == "__main__":
    main()
