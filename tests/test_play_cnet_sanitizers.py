"""The conv net's move under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program (tests/host/play_cnet_san_main.cpp; nothing is loaded into
Python and nothing is preloaded) reads one small case from stdin -- 6 x 6, 15 rows,
C = 64, B = 1 --, packs it into a heap blob of exactly the reported size, computes
the rows' moves (argmax, always sampling, and sampling below the rows' median disc
count) into arrays of exactly R elements and prints them; the output is compared
with tests/play_net_ref.py over tests/cnet_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cnet_cases as cc
import cnet_ref as cr
import play_net_ref as pn
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "play_cnet_san_main.cpp")
SEED, ID_BASE, G0 = 0x1234567890ABCDEF, 4000000000, (1 << 40) + 3


def ints(row):
    return " ".join(str(int(x)) for x in row)


def hexes(row):
    return " ".join("%x" % int(x) for x in row)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_play_cnet_under_asan_ubsan(tmp_path):
    n, R, B, C = 6, 15, 1, 64
    gen = np.random.default_rng(4242)
    weights, biases = cc.draw_weights(n, B, C, gen)
    boards, meta, legal = cc.rows(n, R, seed=31)
    shift_stem, shifts, shift_head, ps, vs, _ = cc.fit(n, weights, biases, boards, meta, legal)
    net = cr.ConvNet(n, weights, biases, shift_stem, shifts, shift_head, ps, vs)
    s = oracle.State(n, R)
    s.boards[:], s.meta[:], s.legal[:] = boards, meta, legal
    D = pn.discs(s)
    mid = int(sorted(D)[R // 2])  # the rows' median disc count: rows on both sides of it
    assert (D < mid).any() and (D >= mid).any()
    samples = (0, 257, mid)
    w = np.concatenate([x.reshape(-1) for x in weights])
    b = np.concatenate([x.reshape(-1) for x in biases])
    lines = ["%d %d %d %d %s %d %d %d %d %d %d %d %d" % (n, C, B, shift_stem, ints(list(shifts) + [0] * (16 - 2 * B)),
                                                         shift_head, ps, vs, R, SEED, ID_BASE, G0, len(samples)),
             ints(w), ints(b)]
    for r in range(R):
        lines.append("%d %s %s" % (meta[r], hexes(boards[r]), hexes(legal[r])))
    lines.append(ints(samples))
    g = G0 + np.arange(R, dtype=np.uint64)
    moves = [pn.net_move(net, s, sd, SEED, ID_BASE, g) for sd in samples]
    assert (moves[0] != moves[1]).any() and (moves[2] != moves[0]).any() and (moves[2] != moves[1]).any()
    exe = str(tmp_path / "play_cnet_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = r.stdout.strip().split("\n")
    assert out[-1] == "conv net moves under ASan and UBSan: clean" and len(out) == len(samples) + 1
    for line, sd, mv in zip(out, samples, moves):
        assert line == "%d %s" % (sd, ints(mv))
