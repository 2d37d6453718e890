#!/usr/bin/env python
"""oth_solve on the GPU box: time per call, nodes searched and nodes per second at
65,536 8x8 boards with exactly 6, 8 and 10 empty squares and at 1,024 boards with
12, beside the single-thread rate of the host build of the same search core
(tests/host/solve_host.cpp) on a sample of each batch; and, per shape, the share
of boards whose search ran over the default node budget (status ABORTED).

    python tools/probe_solve.py [--out profiles/solve/probe.json] [--lib another_build.so]

--lib times another build of the library (an A/B arm, e.g. the parent commit's
built in a worktree) in place of the shipped one.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((65536, 6), (65536, 8), (65536, 10), (1024, 12))
N = 8


def host_lib():
    src = os.path.join(ROOT, "tests", "host", "solve_host.cpp")
    lib = os.path.join(ROOT, "tests", "host", "libsolve_host.so")
    hdrs = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("solve.hpp", "root_tasks.hpp", "bitboard.hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, src])
    L = ctypes.CDLL(lib)
    P = ctypes.c_void_p
    L.host_solve.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_int, ctypes.c_uint64, P, P, P, P, P]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve", "probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-boards", type=int, default=64)
    ap.add_argument("--lib", help="another build of the library (an A/B variant)")
    ap.add_argument("--max-nodes", type=int, default=None, help="the budget (default: solve()'s default)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from gymothelloenv_amd import VecOthelloEnv, _lib
    lib = _lib.load_path(a.lib) if a.lib else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    H = host_lib()
    kw = {} if a.max_nodes is None else {"max_nodes": a.max_nodes}
    res = []
    for E, empties in SHAPES:
        env = VecOthelloEnv(E, board_size=N, seed=empties, device=dev, lib=lib)
        env.reset()
        env.step_policy("random", n_plies=N * N - 4 - empties, record=False)  # a ply places a disc
        b, m, lg = env.get_state()
        live = torch.nonzero((m & 2) == 0).flatten()
        pick = live[torch.arange(E, device=dev) % live.numel()]  # games that ended early: a live board's copy instead
        env.set_state(b[pick], m[pick], lg[pick])
        assert bool((env.count_disks().sum(1) == N * N - empties).all())
        out = env.solve(max_empties=empties, status=True, nodes=True, **kw)  # warm-up, and the counts
        torch.cuda.synchronize()
        status, nodes = out[1].cpu().numpy(), out[2].cpu().numpy()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            env.solve(max_empties=empties, status=True, nodes=True, **kw)
            e1.record(stream)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        us = statistics.median(times)
        total = int(nodes.sum())
        # the host build, one thread, on the first boards of the batch
        k = min(a.host_boards, E)
        sb, sm, sl = [t[:k].cpu().numpy() for t in env.get_state()]
        hv, hb = np.zeros(k, np.int32), np.zeros(k, np.int32)
        hm, hs, hn = np.zeros((k, N * N), np.int32), np.zeros(k, np.uint8), np.zeros(k, np.uint64)
        ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        t0 = time.perf_counter()
        H.host_solve(N, k, ptr(sb), ptr(sm), ptr(sl), empties, 2 ** 32 - 1, ptr(hv), ptr(hb), ptr(hm), ptr(hs), ptr(hn))
        host_s = time.perf_counter() - t0
        exact = status[:k] == _lib.OTH_SOLVE_EXACT
        row = {"boards": E, "board_size": N, "empties": empties, "max_nodes": a.max_nodes or "default",
               "call_us": {"median": us, "min": min(times), "max": max(times)}, "nodes": total,
               "nodes_per_s": total / (us * 1e-6), "root_moves": int(env.legal_actions().sum()),
               "aborted_share": float((status == _lib.OTH_SOLVE_ABORTED).mean()),
               "max_nodes_of_a_board": int(nodes.max()),
               "host_boards": k, "host_nodes": int(hn.sum()), "host_nodes_per_s": float(hn.sum()) / host_s,
               "host_equals_device": bool((hn[exact].astype(np.int64) == nodes[:k][exact]).all())}
        print(json.dumps(row), flush=True)
        res.append(row)
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "lib": a.lib or "shipped", "shapes": res},
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
