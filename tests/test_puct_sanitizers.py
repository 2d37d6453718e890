"""The network-guided search's host core under AddressSanitizer and UBSan: a
stand-alone program with its own main (tests/host/puct_host.cpp with
-DPUCT_MAIN; nothing is loaded into Python) runs the 4 x 4, the 8 x 8 full-tree
and the 10 x 10 cases, each board in a workspace of exactly the reported size,
and compares every output with tests/puct_ref.py."""
import os
import shutil
import subprocess

import pytest

import puct_ref as pf

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "puct_host.cpp")
ROWS = [pf.CASES[0], pf.CASES[2], pf.CASES[3]]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_puct_core_under_asan_ubsan(tmp_path):
    assert [c[0] for c in ROWS] == [4, 8, 10] and ROWS[1][4] == 64
    lines, boards = [], 0
    for c in ROWS:
        n, E, sims, C, T = c
        s, run = pf.case(c)
        pf.check_case(c, run)
        visits, sums, best, nodes, status = run.outputs
        lines.append("%d %d %d %d %d" % c)
        for e in range(E):
            words = " ".join("%x" % int(w) for w in list(s.boards[e]) + list(s.legal[e]))
            nums = " ".join(str(int(x)) for x in list(visits[e]) + list(sums[e]))
            lines.append("%d %d %d %d %s %s" % (s.meta[e], status[e], best[e], nodes[e], words, nums))
            boards += 1
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "puct_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DPUCT_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d boards of %d cases clean" % (boards, len(ROWS)) in r.stdout
