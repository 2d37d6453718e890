"""The batch calls' core under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/puct_batch_san_main.cpp; nothing is loaded into
Python) runs the 8 x 8 full-tree case with K = 4 and one re-root move on a heap
workspace of exactly the reported size and leaf arrays of exactly E K rows, and
compares with tests/puct_batch_ref.py."""
import os
import shutil
import subprocess

import pytest

import puct_batch_ref as pb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "puct_batch_san_main.cpp")
CASE = (8, 12, 150, 320, 64, 4)


def hexes(row):
    return " ".join("%x" % int(x) for x in row)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_puct_batch_under_asan_ubsan(tmp_path):
    n, E, sims, C, T, K = CASE
    assert CASE in pb.CASES
    s, g = pb.game((n, E, sims, 1, C, T, K))
    _, run = pb.case(CASE)
    mv = g.moves[0]
    assert mv["launches"] == len(run.leaves) - 1 and g.counters["collisions"] > 0 and mv["kept"].any()
    lines = ["%d %d %d %d %d %d %d" % (CASE + (mv["launches"],))]
    for e in range(E):
        lines.append("%d %s %s" % (int(s.meta[e]), hexes(s.boards[e]), hexes(s.legal[e])))
    for i in range(mv["launches"]):
        lines.append(" ".join(str(int(k)) for k in g.leaves[i + 1][0]))
    visits, _, best, nodes, status = mv["results"]
    for e in range(E):
        lines.append("%d %d %d %s" % (status[e], best[e], nodes[e], " ".join(str(int(v)) for v in visits[e])))
    lines.append(str(2 * sims))
    st = mv["state"]
    for e in range(E):
        lines.append("%d %d %s %s %d %d" % (mv["actions"][e], int(st.meta[e]), hexes(st.boards[e]), hexes(st.legal[e]),
                                            mv["kept"][e], mv["used"][e]))
    lines.append(" ".join(str(int(k)) for k in g.leaves[-1][0]))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "puct_batch_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1 cases clean" in r.stdout
