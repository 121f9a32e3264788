#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python scripts/isa_same.py OLD_TREE NEW_TREE [file.hip ...]

Every s2d_amd/csrc/*.hip of both trees (or only the named ones) is compiled to assembly the way isa_lint does, with this tree's
build flags, and for every function symbol the instruction stream and the .amdhsa_* block (registers, LDS, scratch) are compared.
Comments and the random __hip_cuid_* lines are dropped and local labels are renumbered in order of appearance, so only a change
of machine code shows.  One line per kernel, `same` or `differs`; the exit status is non-zero on any difference.
"""
import concurrent.futures as cf
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_lint import disassemble

FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
LABEL = re.compile(r"\.L\w+")


def kernels(text):
    """{symbol: normalised lines of its body and of its .amdhsa_kernel block}"""
    names = {m.group(1) for m in map(FUNC.match, text.split("\n")) if m}
    out, cur = {}, None
    for line in text.split("\n"):
        s = line.split(";")[0].strip()
        if not s or "__hip_cuid_" in s:
            continue
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur = out.setdefault(s[:-1], [])
            elif s.startswith(".amdhsa_kernel "):
                cur = out.setdefault(s.split()[1], [])
            continue
        if s.startswith(".Lfunc_end") or s == ".end_amdhsa_kernel":
            cur = None
            continue
        cur.append(s)
    for name, lines in out.items():
        ids = {}
        out[name] = [LABEL.sub(lambda m: ids.setdefault(m.group(0), f".L{len(ids)}"), s) for s in lines]
    return out


def main(argv):
    old, new = (os.path.join(os.path.abspath(t), "s2d_amd", "csrc") for t in argv[:2])
    files = argv[2:] or sorted({os.path.basename(f) for t in (old, new) for f in glob.glob(os.path.join(t, "*.hip"))})
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        asm = list(ex.map(lambda p: kernels(disassemble(p)) if os.path.exists(p) else {},
                          [os.path.join(t, f) for f in files for t in (old, new)]))
    bad = 0
    for i, f in enumerate(files):
        a, b = asm[2 * i], asm[2 * i + 1]
        for k in sorted(set(a) | set(b)):
            same = a.get(k) == b.get(k)
            bad += not same
            print(f"{f} {k} {'same' if same else 'differs'}")
    print(f"isa_same: {len(files)} file(s), {bad} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
