"""The replay store's core under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/replay_san_main.cpp; nothing is loaded into
Python) runs one small case -- 6 x 6, E = 3, H = 4, one full game whose ring
wraps, a gather of every row under all eight symmetries, one sample -- on heap
buffers of exactly the reported sizes, and compares with tests/replay_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import replay_cases as rc
import replay_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "replay_san_main.cpp")
N, E, H = 6, 3, 4
B = 8 * (E * H + 1)
SAMPLE = (1, 2 ** 64 - 3, 2 ** 32 - 2, 2 ** 40 + 1, 24)  # augment, seed, id_key, counter, rows


def hexes(row):
    return " ".join("%x" % int(x) for x in row)


def ints(row):
    return " ".join(str(int(x)) for x in row)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_replay_under_asan_ubsan(tmp_path):
    nn = N * N
    game, ref, gen = rc.OracleGame(N, E, 0, 2), rr.Store(N, E, H), np.random.default_rng(9)
    moves = []
    for m in range(nn):
        s = game.state()
        if (s.meta & 2).all():
            break
        visits = rr.synthetic_visits(E, m, nn)
        skip = (np.arange(E) % 4 == 1).astype(np.uint8)
        ref.append(s, visits, skip if m % 2 else None)
        before = s.copy()
        rewards, dones = game.step(rc.random_legal(s, gen))
        ref.label(rewards, dones)
        for e in range(E):
            moves.append("%d %s %s %d %d %d %s" % (int(before.meta[e]), hexes(before.boards[e]), hexes(before.legal[e]),
                                                   skip[e], rewards[e], dones[e], ints(visits[e])))
    n_moves = len(moves) // E
    assert (game.state().meta & 2).all(), "the game did not end"
    assert max(ref.count) > 2 * H and ref.counts()[2] > 0, "the ring did not wrap, or nothing is labelled"
    lines = ["%d %d %d %d %d" % (N, E, H, B, n_moves)] + moves
    rows = np.tile(np.arange(E * H + 1, dtype=np.int32), 8)  # every row and the first one past the store
    sym = np.repeat(np.arange(8, dtype=np.uint8), E * H + 1)
    want = ref.gather(rows, sym)
    lines.append(str(rows.size))
    for i in range(rows.size):
        lines.append("%d %d %d %d %d %s %s %s" % (rows[i], sym[i], want.state[i], want.meta[i], want.outcome[i],
                                                  hexes(want.boards[i]), hexes(want.legal[i]), ints(want.visits[i])))
    lines.append("%d %d %d %d %d" % SAMPLE)
    drawn = ref.sample(SAMPLE[4], *SAMPLE[:4])
    assert len(set(drawn.rows.tolist())) > 1 and len(set(drawn.sym.tolist())) > 1
    for i in range(SAMPLE[4]):
        lines.append("%d %d %d" % (drawn.rows[i], drawn.sym[i], drawn.outcome[i]))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "replay_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1 cases clean" in r.stdout
