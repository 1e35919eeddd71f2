#!/usr/bin/env python3
"""Are two builds' kernels the SAME machine code?  Disassembles the gfx950 code objects of two .o / .so files and compares
every kernel they share, instruction by instruction (addresses and branch targets stripped).
  python tools/isa_diff_kernels.py A.o B.o [name-filter]  ->  one line per kernel: SAME / DIFF, instruction counts
Used for profiles/r06_asm_loads_ab.json: whether round 5's single-statement hand-written loads changed the headline kernel
at all (they are not called by it: it changed nothing -- the driver-timed -5 % of round 5 was the box)."""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_asm_loads import OBJDUMP, disassemble  # noqa: E402


def kernels(path):
    out, cur = {}, None
    for l in disassemble(path, "gfx950", OBJDUMP):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", l)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if "file format" in l or l.startswith("Disassembly of section"):
            cur = None  # the next code object's header (it names a temporary file) is not part of the last kernel
        if cur is None or not l.strip():
            continue
        t = l.split("//")[0].strip()
        t = re.sub(r"<[^>]*>", "<>", t)
        if t == "...":
            continue  # objdump's stand-in for the zero padding behind a kernel: what follows it decides whether it shows
        if t and not t.endswith(":"):
            # branch offsets are relative: identical code has identical ones; keep the text as is
            out[cur].append(t)
    for code in out.values():
        # s_getpc_b64 s[N:N+1] / s_add_u32 sN, sN, <literal> is the address of a constant table: the literal is the
        # distance from the instruction to the table, which moves whenever ANY kernel or descriptor is added to the file
        for i in range(1, len(code)):
            g = re.match(r"s_getpc_b64 s\[(\d+):\d+\]$", code[i - 1])
            if g:
                code[i] = re.sub(rf"^(s_add_u32 s{g.group(1)}, s{g.group(1)}, )\S+$", r"\1<pc-relative>", code[i])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    rows = []
    for k in sorted(a):
        if k in b and flt in k and not k.startswith("__"):
            rows.append({"kernel": k, "same": a[k] == b[k], "instructions": [len(a[k]), len(b[k])]})
    for r in rows:
        print(("SAME " if r["same"] else "DIFF "), r["instructions"], r["kernel"][:140])
    return rows


if __name__ == "__main__":
    main()
