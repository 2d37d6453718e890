"""The network's move under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/play_net_san_main.cpp; nothing is loaded into
Python) packs one small case -- 6 x 6, 15 rows, one layer of 128 -- into a heap
blob of exactly the reported size, computes the rows' moves (argmax, always
sampling, and sampling below the rows' median disc count) into arrays of exactly R elements and
compares with tests/play_net_ref.py."""
import os
import shutil
import subprocess

import pytest

import net_cases as nc
import play_net_ref as pn
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "play_net_san_main.cpp")
SEED, ID_BASE, G0 = 0x1234567890ABCDEF, 4000000000, (1 << 40) + 3


def ints(row):
    return " ".join(str(int(x)) for x in row)


def hexes(row):
    return " ".join("%x" % int(x) for x in row)


def state_of(c):
    s = oracle.State(c.n, c.R)
    s.boards[:], s.meta[:], s.legal[:] = c.boards, c.meta, c.legal
    return s


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_play_net_under_asan_ubsan(tmp_path):
    c = nc.case(nc.TABLE.index((6, 15, 1, 128)))
    w, b = nc.flat_weights(c)
    shifts = list(c.shifts) + [0] * (4 - c.L)
    s = state_of(c)
    D = pn.discs(s)
    mid = int(sorted(D)[c.R // 2])  # the rows' median disc count: rows on both sides of it
    assert (D < mid).any() and (D >= mid).any()
    samples = (0, 257, mid)
    lines = ["%d %d %d %s %d %d %d %d %d %d %d" % (c.n, c.L, c.H, ints(shifts), c.policy_shift, c.value_shift, c.R, SEED,
                                                   ID_BASE, G0, len(samples)), ints(w), ints(b)]
    for r in range(c.R):
        lines.append("%d %s %s" % (c.meta[r], hexes(c.boards[r]), hexes(c.legal[r])))
    g = G0 + pn.np.arange(c.R, dtype=pn.np.uint64)
    moves = [pn.net_move(c.net, s, sd, SEED, ID_BASE, g) for sd in samples]
    assert (moves[0] != moves[1]).any() and (moves[2] != moves[0]).any() and (moves[2] != moves[1]).any()
    for sd, mv in zip(samples, moves):
        lines.append("%d %s" % (sd, ints(mv)))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "play_net_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1 cases clean" in r.stdout
