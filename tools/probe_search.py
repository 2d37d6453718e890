#!/usr/bin/env python
"""oth_search on the GPU box.

Time: 65,536 random-play 8x8 boards with exactly 30 and with 20 empty squares,
depths 1-5, the default weights: milliseconds per call, nodes per second, the
largest per-board node count and the share of boards over the default node
budget (status ABORTED).  Beside it, as context only, oth_policy_actions(
MAXIMIN(d)) on the same boards and depths: another evaluation (the disc count)
and no pruning.

Strength: win / draw / loss counts of search_actions(depth = 1..4), the default
weights, over 4,096 games each against the device's random, greedy and
MaxiMin-3 movers (oth_step_vs's embedded opponents), colours split evenly, after
6 random opening plies a game (initial_rand_steps: without them a deterministic
opponent replays one game per colour).  Recorded, not asserted.

    python tools/probe_search.py [--out profiles/search/probe.json] [--skip-strength] [--skip-time]
        [--lib another_build.so]

--lib times another build of the library (an A/B arm) in place of the shipped one.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8
BOARDS = 65536
EMPTIES = (30, 20)
DEPTHS = (1, 2, 3, 4, 5)
GAMES = 4096
OPPONENTS = ("random", "greedy", "maximin3")
STRENGTH_DEPTHS = (1, 2, 3, 4)
OPENING_PLIES = 6  # initial_rand_steps of the strength games


def timed(torch, stream, fn, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def time_part(torch, a):
    from gymothelloenv_amd import OthelloLibError, VecOthelloEnv, _lib
    lib = _lib.load_path(a.lib) if a.lib else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = []
    for empties in EMPTIES:
        env = VecOthelloEnv(BOARDS, board_size=N, seed=empties, device=dev, lib=lib)
        env.reset()
        env.step_policy("random", n_plies=N * N - 4 - empties, record=False)  # a ply places a disc
        b, m, lg = env.get_state()
        live = torch.nonzero((m & 2) == 0).flatten()
        pick = live[torch.arange(BOARDS, device=dev) % live.numel()]  # games that ended early: a live board's copy
        env.set_state(b[pick], m[pick], lg[pick])
        assert bool((env.count_disks().sum(1) == N * N - empties).all())
        for depth in DEPTHS:
            out = env.search(depth, status=True, nodes=True)  # warm-up, and the counts
            torch.cuda.synchronize()
            status, nodes = out[1].cpu().numpy(), out[2].cpu().numpy()
            ms = timed(torch, stream, lambda: env.search(depth, status=True, nodes=True), a.reps)
            total = int(nodes.sum())
            row = {"boards": BOARDS, "board_size": N, "empties": empties, "depth": depth, "call_ms": ms,
                   "nodes": total, "nodes_per_s": total / (ms["median"] * 1e-3),
                   "root_moves": int(env.legal_actions().sum()), "max_nodes_of_a_board": int(nodes.max()),
                   "aborted_share": float((status == _lib.OTH_SEARCH_ABORTED).mean())}
            if depth <= a.maximin_depth:
                try:  # context only: the parent's engine on the same boards
                    env.policy_actions("maximin%d" % depth)
                    row["maximin_call_ms"] = timed(torch, stream, lambda: env.policy_actions("maximin%d" % depth), 1)
                except OthelloLibError as err:
                    row["maximin_call_ms"] = "refused: %s" % str(err)[-120:]
            print(json.dumps(row), flush=True)
            rows.append(row)
        env.close()
    return rows


def strength_part(torch, a):
    from gymothelloenv_amd import VecOthelloEnv, _lib
    lib = _lib.load_path(a.lib) if a.lib else None
    dev = torch.device("cuda", 0)
    rows = []
    prot = torch.where(torch.arange(GAMES) % 2 == 0, 1, -1).to(torch.int8)  # white, black, white, ...
    for opp in OPPONENTS:
        for depth in STRENGTH_DEPTHS:
            t0 = time.time()
            # random opening plies: without them two deterministic movers play two games, one per colour
            env = VecOthelloEnv(GAMES, board_size=N, seed=100 + depth, initial_rand_steps=OPENING_PLIES, device=dev,
                                lib=lib)
            env.reset_vs(opp, protagonist=prot)
            calls = 0
            while not bool(env.terminated().all()):
                env.step_vs(env.search_actions(depth=depth), opp, protagonist=prot, observe=False)
                calls += 1
                assert calls <= N * N
            w, d, l = [int(x) for x in env.counts_vs().cpu()]
            assert w + d + l == GAMES
            row = {"games": GAMES, "board_size": N, "search_depth": depth, "opponent": opp,
                   "opening_plies": OPENING_PLIES, "wins": w, "draws": d,
                   "losses": l, "seconds": time.time() - t0}
            print(json.dumps(row), flush=True)
            rows.append(row)
            env.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--maximin-depth", type=int, default=5, help="the deepest MaxiMin timed beside the search")
    ap.add_argument("--lib", help="another build of the library (an A/B variant)")
    ap.add_argument("--skip-time", action="store_true")
    ap.add_argument("--skip-strength", action="store_true")
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "lib": a.lib or "shipped"}
    if not a.skip_time:
        res["time"] = time_part(torch, a)
    if not a.skip_strength:
        res["strength"] = strength_part(torch, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
