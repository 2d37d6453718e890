"""The root noise's core under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/noise_san_main.cpp; nothing is loaded into Python)
runs cases of tests/noise_cases.py -- one to four words a board, both modes, in place
and not, a table whose entries are clamped, the largest counter -- on heap buffers of
exactly the sizes the call is given, and compares with tests/noise_ref.py."""
import os
import shutil
import subprocess

import pytest

import noise_cases as nz

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "noise_san_main.cpp")
CASES = [(dict(n=4, K=1, mode="root"), False, 64), (dict(n=6, K=3, mode="leaf"), True, 256),
         (dict(n=10, K=3, mode="leaf"), False, 1), (dict(n=13, K=1, mode="root"), True, 0),
         (dict(n=16, K=3, mode="leaf"), True, 64), (dict(nz.SPECIAL[1][1]), False, 64),
         (dict(nz.SPECIAL[6][1]), True, 256), (dict(nz.SPECIAL[4][1]), False, 256)]


def hexes(a):
    return " ".join("%x" % int(x) for x in a.ravel())


def ints(a):
    return " ".join(str(int(x)) for x in a.ravel())


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_noise_under_asan_ubsan(tmp_path):
    lines = []
    for kw, inplace, epsilon in CASES:
        c = nz.make(**kw)
        want, _ = nz.expected(c, epsilon)
        leaf = c.kind is not None
        lines.append("%d %d %d %d %d %d %d %d %d" % (c.n, nz.E, c.K, leaf, inplace, epsilon, c.seed,
                                                     (c.id_key + c.id_base) % 2 ** 32, c.counter))
        lines.append(hexes(c.table))
        for e in range(nz.E):
            lines.append(hexes(c.handle_boards[e]) + " " + hexes(c.handle_legal[e]))
        if leaf:
            for r in range(nz.E * c.K):
                lines.append("%d %s" % (c.kind[r], hexes(c.boards[r])))
        lines.append(ints(c.priors))
        lines.append(ints(want))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "noise_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d cases clean" % len(CASES) in r.stdout
