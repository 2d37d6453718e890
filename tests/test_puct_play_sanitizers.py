"""The host core of oth_puct_pick and oth_puct_reroot under AddressSanitizer and UBSan:
a stand-alone program with its own main (tests/host/puct_play_host.cpp with
-DPUCT_PLAY_MAIN; nothing is loaded into Python) plays the 4 x 4, the 8 x 8
full-tree and the 10 x 10 games of tests/puct_play_ref.py board by board, each
board in a workspace of exactly the reported size, and compares the picks, the
visits, kept, tree_nodes and the leaf after every re-root."""
import os
import shutil
import subprocess

import pytest

import puct_play_ref as pp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "puct_play_host.cpp")
ROWS = [pp.CASES[0], pp.CASES[2], pp.CASES[4]]


def hexes(words):
    return " ".join("%x" % int(w) for w in words)


def ints(xs):
    return " ".join(str(int(x)) for x in xs)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pick_and_reroot_under_asan_ubsan(tmp_path):
    assert [c[0] for c in ROWS] == [4, 8, 10] and ROWS[1][5] == 64
    lines, boards = [], 0
    for c in ROWS:
        n, E, S, M, C, T = c
        s, game = pp.case(c)
        pp.check_case(c, game)
        lines.append("%d %d %d %d %d %d %d %d" % (c + (pp.SEED, pp.ID_KEY)))
        for e in range(E):
            lines.append("%d %d %d %s" % (e, game.sample[e], s.meta[e], hexes(list(s.boards[e]) + list(s.legal[e]))))
            at = 0
            for m, mv in enumerate(game.moves):
                at += S + 1  # the leaves after this move's re-root
                kind, _, lmeta, _ = game.leaves[at]
                visits, _, best, nodes, _ = mv["results"]
                st, rp = mv["state"], mv["root_priors"]
                lines.append(" ".join([
                    "%d %d %d %d" % (mv["counter"], mv["picks"][e], best[e], nodes[e]), ints(visits[e]),
                    "%d %d" % (mv["actions"][e], st.meta[e]), hexes(list(st.boards[e]) + list(st.legal[e])),
                    "0" if rp is None else "1 " + ints(rp[e]),
                    "%d %d %d %d" % (mv["kept"][e], mv["used"][e], kind[e], lmeta[e])]))
            boards += 1
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "puct_play_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DPUCT_PLAY_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d boards of %d cases clean" % (boards, len(ROWS)) in r.stdout
