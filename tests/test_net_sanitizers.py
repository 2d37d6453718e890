"""The network's core under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/net_san_main.cpp; nothing is loaded into Python)
packs one small case -- 6 x 6, 15 rows, one layer of 128 -- into a heap blob of
exactly the reported size, evaluates it into arrays of exactly R rows and compares
with tests/net_ref.py."""
import os
import shutil
import subprocess

import pytest

import net_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "net_san_main.cpp")


def ints(row):
    return " ".join(str(int(x)) for x in row)


def hexes(row):
    return " ".join("%x" % int(x) for x in row)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_net_under_asan_ubsan(tmp_path):
    c = nc.case(nc.TABLE.index((6, 15, 1, 128)))
    w, b = nc.flat_weights(c)
    shifts = list(c.shifts) + [0] * (4 - c.L)
    lines = ["%d %d %d %s %d %d %d" % (c.n, c.L, c.H, ints(shifts), c.policy_shift, c.value_shift, c.R), ints(w), ints(b)]
    for r in range(c.R):
        lines.append("%d %s %s" % (c.meta[r], hexes(c.boards[r]), hexes(c.legal[r])))
    for r in range(c.R):
        lines.append("%d %s %s" % (c.values[r], ints(c.priors[r]), ints(c.logits[r])))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "net_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1 cases clean" in r.stdout
