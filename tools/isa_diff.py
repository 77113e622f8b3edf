#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two versions of csrc/art_kernels.hip (no GPU needed):

    python tools/isa_diff.py [BASE_REV] [--show NAME]

BASE_REV (default HEAD~1) is taken from git (`git archive` of csrc/ and include/), the other side is the working tree.
Both are compiled with `hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only`; each kernel's instructions
are compared with comments, directives and labels stripped (branch targets renamed).  Prints the kernels that are
identical, changed, removed and added; exit status 1 if any kernel of BASE_REV changed or disappeared."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = os.path.join("attosecondraytracing_amd", "csrc", "art_kernels.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"]


def kernels(asm):
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        body = []
        for line in m.group(2).split("\n"):
            line = line.split(";")[0].rstrip()
            t = line.strip()
            if not t or t.startswith(".") and (t.endswith(":") or re.match(r"^\.\w", t)) or re.match(r"^\.?L\w*:$", t):
                continue
            body.append(re.sub(r"\.LBB\d+_\d+", "L", line))
        out[m.group(1)] = body
    return out


def compile_tree(root, td, tag):
    out = os.path.join(td, tag + ".s")
    subprocess.check_call(["hipcc"] + FLAGS + ["-o", out, os.path.join(root, REL)], stderr=subprocess.DEVNULL)
    return kernels(open(out).read())


def main():
    args = sys.argv[1:]
    show = None
    if "--show" in args:
        k = args.index("--show")
        show = args[k + 1]
        del args[k:k + 2]
    rev = args[0] if args else "HEAD~1"
    with tempfile.TemporaryDirectory() as td:
        base = os.path.join(td, "base")
        os.makedirs(base)
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, "attosecondraytracing_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
        a = compile_tree(base, td, "base")
        b = compile_tree(ROOT, td, "work")
    same = [k for k in a if k in b and a[k] == b[k]]
    changed = [k for k in a if k in b and a[k] != b[k]]
    removed = [k for k in a if k not in b]
    added = [k for k in b if k not in a]
    print(f"{rev}: {len(a)} kernels; working tree: {len(b)} kernels")
    print(f"identical: {len(same)}  changed: {len(changed)}  removed: {len(removed)}  added: {len(added)}")
    for tag, lst in (("changed", changed), ("removed", removed), ("added", added)):
        for k in lst:
            print(f"  {tag}: {k}")
    if show:
        for k in a:
            if show in k and k in b:
                import difflib
                sys.stdout.writelines(difflib.unified_diff([l + "\n" for l in a[k]], [l + "\n" for l in b[k]], rev, "work"))
    return 1 if changed or removed else 0


if __name__ == "__main__":
    sys.exit(main())
