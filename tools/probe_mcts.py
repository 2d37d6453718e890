#!/usr/bin/env python3
"""oth_mcts against oth_playouts playing the same number of playouts from the
same boards, on the GPU box:

  tree   VecOthelloEnv.mcts(I, playouts=R): I R playouts a board, one node at a
         time, with the tree's descent and backup between them
  flat   VecOthelloEnv.playouts(...) in ROOT mode, I R playouts a board from the
         root (in calls of at most 65,536 a board)

for two shapes from positions 20 plies into random 8x8 games: 8,192 boards at
I = 64, R = 8 (every lane plays, eight boards a wave) and one board at I = 4,096,
R = 64 (a whole wave a board: leaf parallelism only).  The flat side is the
playout throughput the device has for that many games; what the tree side loses
against it is the serial tree work of each board's leader lane plus the waiting
of a wave's lanes for its longest game.  (The tree's playouts start deeper than
the root, so they are somewhat shorter: the ratio flatters the tree a little.)
Times are medians over bursts between device events, after a warm-up of both
sides.  One more figure bounds the split inside an iteration: playouts(R) alone,
R games a board from the root on the same lanes, against the search's time per
iteration.  The distribution of tree_nodes says what max_tree_nodes a call needs.

A second part plays whole games as black against the device's random policy on
256 6x6 boards and against its greedy policy on 256 8x8 boards, one call per
move: mcts (I = 64, R = 8: 512 playouts a move) and flat Monte-Carlo
(playout_actions at 64 playouts per possible move, about as many) -- the win
rates of DESIGN.md section 5.

    python tools/probe_mcts.py [--out profiles/mcts.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8192, 64, 8), (1, 4096, 64))
SEED, COUNTER, N = 2024, 5, 8
FLAT_MAX = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcts.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=3)
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import VecOthelloEnv
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            for _ in range(a.burst):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / a.burst)
        return statistics.median(out), min(out), max(out)

    res = []
    for E, I, R in SHAPES:
        env = VecOthelloEnv(E, board_size=N, seed=1, env_id_base=1000, device=dev)
        env.step_policy("random", n_plies=20, record=False)
        live = int((~env.terminated()).sum())
        total = I * R  # playouts a board
        chunks = [FLAT_MAX] * (total // FLAT_MAX) + ([total % FLAT_MAX] if total % FLAT_MAX else [])
        T = max(N * N, I * (N * N - 4) // 4)  # VecOthelloEnv.mcts' default

        def tree():
            return env.mcts(I, playouts=R, max_tree_nodes=T, seed=SEED, counter=COUNTER, wins2=True, tree_nodes=True,
                            status=True)

        def flat():
            return [env.playouts(c, seed=SEED, counter=COUNTER + j) for j, c in enumerate(chunks)]

        vis, w2, tn, st = tree()  # warm-up of both sides
        wdl = sum(flat())
        assert int(vis.sum()) == live * I and int(wdl.sum()) == live * total
        tt, tf = timed(tree), timed(flat)
        # one iteration's playouts alone: R games a board from the root on the same lanes (the longest
        # games of the search, and a launch of their own: an upper bound of an iteration's playout time)
        t1 = timed(lambda: env.playouts(R, seed=SEED, counter=COUNTER))
        nodes = tn[st == 0].to(torch.float64).cpu()
        q = torch.quantile(nodes, torch.tensor([0.0, 0.5, 0.9, 0.99, 1.0], dtype=torch.float64)).tolist()
        # the root's value both ways, from the side to move: (2 wins + draws) / (2 playouts)
        tree_value = float(w2.sum()) / (2.0 * live * total)
        flat_value = float(2 * wdl[:, 0].sum() + wdl[:, 1].sum()) / (2.0 * live * total)
        row = {"boards": E, "iterations": I, "playouts": R, "board_size": N, "live_boards": live,
               "playouts_per_board": total, "max_tree_nodes": T,
               "mcts_us": {"median": tt[0], "min": tt[1], "max": tt[2]},
               "playouts_us": {"median": tf[0], "min": tf[1], "max": tf[2]},
               "mcts_playouts_per_s": live * total / (tt[0] * 1e-6),
               "flat_playouts_per_s": live * total / (tf[0] * 1e-6),
               "mcts_over_flat_time": tt[0] / tf[0],
               "mcts_us_per_iteration": tt[0] / I,
               "one_iteration_playouts_us": {"median": t1[0], "min": t1[1], "max": t1[2]},
               "tree_nodes": {"min": q[0], "median": q[1], "p90": q[2], "p99": q[3], "max": q[4],
                              "mean": float(nodes.mean())},
               "boards_with_a_full_tree": int((tn[st == 0] > T - (N * N - 4)).sum()),
               "root_value_tree": tree_value, "root_value_flat": flat_value}
        print(json.dumps(row), flush=True)
        res.append(row)
        env.close()
        torch.cuda.empty_cache()

    games = []
    for n, opp, E in ((6, "random", 256), (8, "greedy", 256)):
        for who in ("mcts", "flat"):
            env = VecOthelloEnv(E, board_size=n, seed=11, device=dev)
            env.reset_vs(opp, protagonist=-1)
            done = torch.zeros(E, dtype=torch.bool, device=dev)
            for move in range(n * n):
                if bool(done.all()):
                    break
                if who == "mcts":
                    act = env.mcts_actions(64, playouts=8, seed=5, counter=move)
                else:
                    act = env.playout_actions(64, seed=5, counter=move)
                done |= env.step_vs(act, opp, observe=False)[2]
            assert bool(done.all())
            d = env.count_disks()  # (white, black)
            row = {"board_size": n, "opponent": opp, "boards": E, "black": who,
                   "wins": int((d[:, 1] > d[:, 0]).sum()), "draws": int((d[:, 1] == d[:, 0]).sum()),
                   "losses": int((d[:, 1] < d[:, 0]).sum())}
            print(json.dumps(row), flush=True)
            games.append(row)
            env.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "burst": a.burst, "shapes": res,
                   "games": games}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
