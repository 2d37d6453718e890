"""select64_tab (csrc/bitboard.hpp: the play kernels' pick -- the k-th set bit of
a word by sign masks, no compare and no select, the bit inside its byte from the
rank-reversed sel8 table) compiled for the host with g++ as a stand-alone
program (tests/host/select_host.cpp), against select64 (the nibble form) and
the k-th set bit itself, for every k < popcount of: all 2^16 patterns in each
16-bit quarter (alone and over a background), every single-bit word, the full
word, 5^8 words whose bytes are empty, hold 1, 2 or 7 bits or are full (k on
both sides of every byte-prefix count), and 10^6 drawn words; once plain and
once under -fsanitize=undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "select_host.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags
                          + ["-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "clean" in r.stdout
    return r.stdout


def test_select64_tab_every_rank(tmp_path):
    out = build_and_run(tmp_path, "select_main", ["-O2"])
    words = int(out.split(":")[1].split()[0])
    assert words == 2 * 4 * 65536 + 2 * 64 + 1 + 5 ** 8 + 10 ** 6, out


def test_select64_tab_under_ubsan(tmp_path):
    """The same program with every shift count, index and conversion checked."""
    build_and_run(tmp_path, "select_main_ubsan",
                  ["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-static-libubsan"],
                  env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
