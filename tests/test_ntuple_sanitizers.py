"""The n-tuple network's core under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/ntuple_san_main.cpp; nothing is loaded into Python)
runs cases of tests/ntuple_cases.py -- one to four words a board, the three kinds of
lengths, evaluations, updates with the largest rate, a zero rate and a weight that
wraps (the additions are unsigned), and searches with and without a budget -- on heap
buffers of exactly the sizes the calls are given, and compares with tests/ntuple_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ntuple_cases as nc
import ntuple_ref as nr
import search_ref as sh
import solve_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "ntuple_san_main.cpp")
EVALS = [((4, 1, "eights"), 0, 65), ((6, 32, "ones"), 9, 64), ((10, 5, "mixed"), 0, 257), ((13, 32, "mixed"), 9, 63),
         ((16, 32, "eights"), 0, 65), ((8, 5, "mixed"), 0, 1)]
UPDATES = [((4, 32, "ones"), 0, 257, 5000, 12), ((8, 5, "mixed"), 0, 257, 1 << 24, 0), ((10, 32, "mixed"), 9, 65, 0, 7),
           ((16, 5, "mixed"), 9, 64, 1 << 24, 40), ((13, 1, "eights"), 0, 63, 1, 1)]
SEARCHES = [(4, 4, 1 << 22), (8, 3, 1 << 22), (10, 2, 1 << 22), (16, 2, 1 << 22), (8, 3, 4)]  # (n, depth, max_nodes)
SEARCH_ROWS = 20


def hexes(a):
    return " ".join("%x" % int(x) for x in np.asarray(a).ravel())


def ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def head(kind, n, tp, shift, R, weights, boards, meta):
    lines = ["%d %d %d %d %d" % (kind, n, len(tp), shift, R)]
    lines += ["%d %s" % (len(t), ints(t)) for t in tp]
    lines.append(ints(weights))
    lines += ["%s %d" % (hexes(boards[r]), int(meta[r])) for r in range(R)]
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ntuple_under_asan_ubsan(tmp_path):
    lines, cases = [], 0
    for cfg, shift, R in EVALS:
        c = nc.case(*cfg)
        v, s = nr.evaluate(c.n, c.tuples, shift, c.weights, c.boards[:R], c.meta[:R])
        lines += head(0, c.n, c.tuples, shift, R, c.weights, c.boards, c.meta) + [ints(v), ints(s)]
        cases += 1
    for cfg, shift, R, rate, rate_shift in UPDATES:
        c = nc.case(*cfg)
        w, d = nr.update(c.n, c.tuples, shift, c.weights, c.boards[:R], c.meta[:R], c.targets[:R], rate, rate_shift)
        lines += head(1, c.n, c.tuples, shift, R, c.weights, c.boards, c.meta)
        lines += ["%d %d" % (rate, rate_shift), ints(c.targets[:R]), ints(d), ints(w)]
        cases += 1
    # a weight that wraps: every row hits the same three entries, all at 2^31 - 5
    c = nc.case(4, 1, "ones")
    wrap = np.full(4, 2 ** 31 - 5, dtype=np.int32)
    tg = np.full(257, 40000, dtype=np.int32)
    w, d = nr.update(4, [[5]], 24, wrap, c.boards, c.meta, tg, 1, 0)
    assert (d > 0).all() and (w < 0).all()
    lines += head(1, 4, [[5]], 24, 257, wrap, c.boards, c.meta) + ["1 0", ints(tg), ints(d), ints(w)]
    cases += 1
    for n, depth, max_nodes in SEARCHES:
        s = sr.subset(sh.batch(n, 74)[0], np.arange(SEARCH_ROWS))
        c = nc.case(n, 5, "mixed")
        res = nr.search(s, depth, c.tuples, 3, c.weights, terminal=64, max_nodes=max_nodes)
        assert (res.status == sh.ABORTED).any() == (max_nodes == 4)
        lines += head(2, n, c.tuples, 3, s.E, c.weights, s.boards, s.meta)
        lines += ["%d 64 %d" % (depth, max_nodes), hexes(s.legal)]
        for e in range(s.E):
            lines.append("%d %d %d %d %s" % (res.value[e], res.best[e], res.status[e], res.nodes[e], ints(res.move_values[e])))
        cases += 1
    text = tmp_path / "cases.txt"
    text.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "ntuple_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(text)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d cases clean" % cases in r.stdout
