"""The convolutional network's core under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program (tests/host/cnet_san_main.cpp;
nothing is loaded into Python) packs one small case -- 6 x 6, 15 rows, B = 1, C = 64
-- into a heap blob of exactly the reported size, evaluates it into arrays of exactly R
rows and compares with tests/cnet_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cnet_cases as cc
import cnet_ref as cr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "cnet_san_main.cpp")


def ints(row):
    return " ".join(str(int(x)) for x in row)


def hexes(row):
    return " ".join("%x" % int(x) for x in row)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cnet_under_asan_ubsan(tmp_path):
    n, R, B, C = 6, 15, 1, 64
    big = cc.case(cc.TABLE.index((6, 15, 2, 128)))  # its rows: games and the hand-made ones
    boards, meta, legal = big.boards, big.meta, big.legal
    weights, biases = cc.draw_weights(n, B, C, np.random.default_rng(99))
    shift_stem, shifts, shift_head, ps, vs, census = cc.fit(n, weights, biases, boards, meta, legal)
    assert min(census) >= 0.25
    priors, values, logits = cr.ConvNet(n, weights, biases, shift_stem, shifts, shift_head, ps, vs).evaluate(boards, meta,
                                                                                                             legal)
    w = np.concatenate([x.reshape(-1) for x in weights])
    b = np.concatenate([x.reshape(-1) for x in biases])
    lines = ["%d %d %d %d %s %d %d %d %d" % (n, C, B, shift_stem, ints(list(shifts) + [0] * (16 - 2 * B)), shift_head, ps,
                                               vs, R), ints(w), ints(b)]
    for r in range(R):
        lines.append("%d %s %s" % (meta[r], hexes(boards[r]), hexes(legal[r])))
    for r in range(R):
        lines.append("%d %s %s" % (values[r], ints(priors[r]), ints(logits[r])))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "cnet_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1 cases clean" in r.stdout
