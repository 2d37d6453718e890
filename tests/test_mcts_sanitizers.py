"""The tree search's host core under AddressSanitizer and UBSan: a stand-alone
program with its own main (tests/host/mcts_host.cpp with -DMCTS_MAIN; nothing is
loaded into Python) runs the 4 x 4, the 8 x 8 full-tree and the 10 x 10 cases
and compares every output with tests/mcts_ref.py."""
import os
import shutil
import subprocess

import pytest

import mcts_ref as mr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "mcts_host.cpp")
ROWS = [mr.CASES[0], mr.CASES[2], mr.CASES[4]]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mcts_core_under_asan_ubsan(tmp_path):
    assert [c[0] for c in ROWS] == [4, 8, 10] and ROWS[1][5] == 64
    lines, boards = [], 0
    for c in ROWS:
        n, E, I, R, C, T = c
        s, res = mr.case(c)
        mr.check_case(c, res)
        lines.append("%d %d %d %d %d %d %d %d %d %d" % (n, E, I, R, C, T, mr.SEED, mr.ID_KEY, mr.ID_BASE, mr.COUNTER))
        for e in range(E):
            words = " ".join("%x" % int(w) for w in list(s.boards[e]) + list(s.legal[e]))
            nums = " ".join(str(int(x)) for x in list(res.visits[e]) + list(res.wins2[e]))
            lines.append("%d %d %d %d %s %s" % (s.meta[e], res.status[e], res.best[e], res.tree_nodes[e], words, nums))
            boards += 1
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "mcts_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMCTS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d boards of %d cases clean" % (boards, len(ROWS)) in r.stdout
