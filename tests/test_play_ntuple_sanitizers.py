"""The play-ntuple core under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone
program (tests/host/play_ntuple_san_main.cpp; nothing is loaded into Python) runs the move
T and the TD target of the search batch's boards -- one-, two- and four-word boards, a
budget that aborts, endgame mode, exploring plies with a 64-bit seed and ids past 2^32 --
on heap buffers of exactly the sizes the call is given, and compares with
tests/play_ntuple_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import play_ntuple_ref as pn
import rng_ref as rr
import search_ref as sh
import solve_ref as sr
from test_play_ntuple_host import ID_BASE, SEED, policies, reference_targets

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "play_ntuple_san_main.cpp")
ROWS = 30
CASES = [(4, 0, 0), (8, 0, 0), (10, 0, 0), (16, 0, 0), (8, 1, 0), (8, 1, 20000), (10, 1, 65536), (4, 0, 30000)]  # (n, side, explore)


def hexes(a):
    return " ".join("%x" % int(x) for x in np.asarray(a).ravel())


def ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_play_ntuple_core_under_asan_ubsan(tmp_path):
    lines, held = [], set()
    for n, side, explore in CASES:
        s = sr.subset(sh.batch(n, 74)[0], np.arange(ROWS))
        p = policies(n)[side]._replace(explore=explore)
        ids = rr.ids_from(ID_BASE, s.E)
        g = np.arange(s.E, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33)
        a, f, ex, end, done = pn.moves(s, p, p, SEED, ids, g)
        t = reference_targets(s, a, done, p)[0]
        held |= {k for k, v in (("fallback", f.any()), ("explored", ex.any()), ("endgame", end.any()), ("target", t.any())) if v}
        lines.append("%d %d %d %d %d %d %d %d %d %d" % (n, len(p.tuples), p.shift, s.E, p.depth, p.terminal,
                                                       p.endgame_empties, p.explore, p.max_nodes, SEED))
        lines += ["%d %s" % (len(tp), ints(tp)) for tp in p.tuples]
        lines.append(ints(p.weights))
        for e in range(s.E):
            lines.append("%s %s %d %d %d %d %d %d %d" % (hexes(s.boards[e]), hexes(s.legal[e]), s.meta[e], ids[e], g[e],
                                                         a[e], f[e], ex[e], t[e]))
    assert held == {"fallback", "explored", "endgame", "target"}
    text = tmp_path / "cases.txt"
    text.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "play_ntuple_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(text)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d cases clean" % len(CASES) in r.stdout
