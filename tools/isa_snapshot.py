#!/usr/bin/env python3
"""Device assembly of every translation unit of the library (the build's own
flags, --cuda-device-only -S) with comments and path/ident lines stripped, one
file per unit, for checking that a source cleanup leaves the generated code
unchanged:

    python tools/isa_snapshot.py /tmp/isa_before
    ... edit ...
    python tools/isa_snapshot.py /tmp/isa_after
    python tools/isa_snapshot.py --compare [--brief] /tmp/isa_before /tmp/isa_after

The compare mode goes kernel symbol by kernel symbol (code and kernel descriptor,
block labels renumbered per function so that a kernel added or removed elsewhere
in the unit does not show up in its neighbours), prints `identical` or the number
of differing lines with the differing lines themselves, and exits non-zero if
anything differs.  --brief counts a unit's identical symbols on one line and
leaves the differing lines out: a record short enough to commit.
"""
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gymothelloenv_amd import build as B  # noqa: E402


def units():
    u = [("capi.hip", "capi", []), ("masked.hip", "masked", [])]
    u += [("kernels_n.hip", "kernels_n%d" % n, ["-DOTH_N=%d" % n]) for n in B.SIZES]
    u += [("play_rand_n.hip", "play_rand_n%d" % n, ["-DOTH_N=%d" % n] + B.play_flags()) for n in B.PLAY_SIZES]
    u += [("playouts_n.hip", "playouts_n%d" % n, ["-DOTH_N=%d" % n] + B.PLAYOUT_FLAGS) for n in B.SIZES]
    for src in ("solve_n", "search_n", "play_search_n"):
        u += [(src + ".hip", "%s%d" % (src, n), ["-DOTH_N=%d" % n]) for n in B.SIZES]
    return u


def clean(text):
    out = []
    for line in text.splitlines():
        s = line.split(";", 1)[0].rstrip() if not line.lstrip().startswith(".") else line.rstrip()
        if not s or s.lstrip().startswith((".ident", ".file", ".amdgpu_hsa", "//")):
            continue
        if "oth-src-sha256" in s or "__hip_cuid" in s:
            continue
        out.append(s)
    return "\n".join(out) + "\n"


def one(u, outdir):
    src, name, defs = u
    tmp = os.path.join(outdir, name + ".raw.s")
    cmd = [B.HIPCC, "--offload-arch=%s" % B.ARCH] + B.BASE_FLAGS + ["-I", os.path.join(ROOT, "include")] + defs + \
        ['-DOTH_SRC_HASH="0"', "--cuda-device-only", "-S", "-o", tmp, os.path.join(B.CSRC, src)]
    subprocess.run(cmd, check=True, cwd=ROOT)
    txt = open(tmp).read()
    os.remove(tmp)
    with open(os.path.join(outdir, name + ".s"), "w") as f:
        f.write(clean(txt))
    return name


_LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+")


def symbols(text):
    """{kernel symbol: its lines}: the function from .type to .size plus its .amdhsa_kernel block."""
    syms, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(_LABEL.sub(lambda g: ".L" + g.group(1), line))
            if re.match(r"\s*(\.size\s|\.end_amdhsa_kernel)", line):
                cur = None
    return syms


def compare(dir_a, dir_b, show=40, brief=False):
    names = sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b)))
    total = differing = 0
    for name in (n for n in names if n.endswith(".s")):
        sides = []
        for d in (dir_a, dir_b):
            path = os.path.join(d, name)
            sides.append(symbols(open(path).read()) if os.path.exists(path) else {})
        same = 0
        for sym in sorted(set(sides[0]) | set(sides[1])):
            a, b = sides[0].get(sym), sides[1].get(sym)
            total += 1
            if a == b:
                same += 1
                if not brief:
                    print("%s %s: identical" % (name[:-2], sym))
                continue
            differing += 1
            if a is None or b is None:
                print("%s %s: only in %s" % (name[:-2], sym, dir_b if a is None else dir_a))
                continue
            delta = [x for x in difflib.unified_diff(a, b, lineterm="", n=0) if not x.startswith(("---", "+++"))]
            print("%s %s: %d lines differ" % (name[:-2], sym, sum(1 for x in delta if x[0] in "+-")))
            if brief:
                continue
            for x in delta[:show]:
                print("    " + x)
            if len(delta) > show:
                print("    ... (%d more)" % (len(delta) - show))
        if brief:
            print("%s: %d of %d symbols identical" % (name[:-2], same, len(set(sides[0]) | set(sides[1]))))
    print("%d kernel symbols compared, %d differ" % (total, differing))
    return 1 if differing else 0


def main():
    if sys.argv[1] == "--compare":
        brief = "--brief" in sys.argv
        dirs = [x for x in sys.argv[2:] if x != "--brief"]
        sys.exit(compare(dirs[0], dirs[1], brief=brief))
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        for name in ex.map(lambda u: one(u, outdir), units()):
            print(name, flush=True)


if __name__ == "__main__":
    main()
