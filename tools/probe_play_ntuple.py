#!/usr/bin/env python
"""oth_play_ntuple on the GPU box: the one launch beside the
composition of the calls that did the same work before it.

At 8x8 with 12 snake tuples of length 6, value_shift 6, at 1,024 and 65,536 boards
(auto-reset, no random openings, no exploring plies), depth 1 and 2:
  (a) a ply of play: play_ntuple, 10 plies a launch, beside 10 x (search_ntuple_actions
      + step);
  (b) a TD round of 10 plies: td_play (play_ntuple with td rows + one masked update over
      the 10 E rows) beside 10 x README's five-call ply (get_state, search_ntuple_actions,
      step, evaluate, update on boards[live]: one host synchronisation a ply).
The two sides of (a) play the same moves: the boards after the first window are compared
before anything is timed.  The two sides of (b) do not hold the same weights afterwards
(one update a round against one a ply): (b) compares what a learner pays for ten plies
of TD data and their updates, and says so.

A timing is `calls` rounds of 10 plies between two device events after a warm-up,
divided by 10 `calls`: microseconds a ply, the host's enqueues inside the window.  Every
window starts from the same saved boards and weights; the two sides alternate inside a
repetition; the median of `reps` windows with min and max.

    python tools/probe_play_ntuple.py [--out profiles/play_ntuple/probe.json] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, PLIES = 8, 10
BOARDS = (1024, 65536)
DEPTHS = (1, 2)
TUPLES, LENGTH, VALUE_SHIFT = 12, 6, 6


def window(torch, stream, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for _ in range(calls):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * PLIES)  # microseconds a ply


def summary(times, calls):
    return {"median": statistics.median(times), "min": min(times), "max": max(times), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "play_ntuple", "probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    from gymothelloenv_amd import NTupleNet, NTuplePlayer, VecOthelloEnv, snake_tuples
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    net = NTupleNet(N, snake_tuples(N, TUPLES, LENGTH, seed=1), VALUE_SHIFT, device=dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    w0 = torch.randint(-20000, 20001, (net.weight_count,), generator=g, dtype=torch.int32).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "board_size": N, "plies_per_launch": PLIES,
           "tuples": TUPLES, "length": LENGTH, "unit": "microseconds a ply", "rows": []}
    for E in BOARDS:
        env = VecOthelloEnv(E, board_size=N, seed=1, auto_reset=True, sudden_death_on_invalid_move=False, device=dev)
        env.reset()
        env.step_policy("random", n_plies=10, record=False)  # ten plies into the games: a dozen root moves a board
        sd = env.state_dict()
        rate, rate_shift = net.rate_for(0.1, E)
        for depth in DEPTHS:
            player = NTuplePlayer(net, depth=depth)

            def restore():
                env.load_state_dict(sd)
                net.weights.copy_(w0)

            def play_fused():
                env.play_ntuple(player, None, PLIES, record=False)

            def play_composed():
                for _ in range(PLIES):
                    env.step(env.search_ntuple_actions(depth=depth, net=net), observe=False)

            def td_fused():
                net.td_play(env, PLIES, rate, rate_shift, depth=depth)

            def td_composed():  # README's five-call ply
                for _ in range(PLIES):
                    boards, meta, _ = env.get_state()
                    live = (meta & 2) == 0
                    _, _, done, _ = env.step(env.search_ntuple_actions(depth=depth, net=net), observe=False)
                    nboards, nmeta, _ = env.get_state()
                    nxt = net.evaluate(nboards, nmeta)
                    target = torch.where(((nmeta ^ meta) & 1) == 0, nxt, -nxt)
                    discs = env.count_disks()
                    mine = (discs[:, 0] - discs[:, 1]) * torch.where((meta & 1) != 0, 1, -1)
                    target = torch.where(done, 32768 * torch.sign(mine), target)
                    net.update(boards[live], meta[live], target[live].int(), rate, rate_shift)

            # the same moves first: the boards after one launch / ten composed plies
            restore()
            play_fused()
            after = [t.clone() for t in env.get_state()]
            restore()
            play_composed()
            same = all(torch.equal(x, y) for x, y in zip(after, env.get_state()))
            calls = 20 if E <= 4096 else 3
            row = {"boards": E, "depth": depth, "same_boards": bool(same)}
            sides = (("play_fused", play_fused), ("play_composed", play_composed), ("td_fused", td_fused),
                     ("td_composed", td_composed))
            for _, fn in sides:  # warm-up of every shape
                restore()
                fn()
            times = {name: [] for name, _ in sides}
            for _ in range(a.reps):
                for name, fn in sides:  # alternating inside a repetition
                    restore()
                    times[name].append(window(torch, stream, fn, calls))
            for name, _ in sides:
                row[name] = summary(times[name], calls)
            row["play_speedup"] = row["play_composed"]["median"] / row["play_fused"]["median"]
            row["td_speedup"] = row["td_composed"]["median"] / row["td_fused"]["median"]
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
