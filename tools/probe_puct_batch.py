#!/usr/bin/env python3
"""The cost of the batch calls of the network-guided tree search
(oth_puct_advance_batch: one lane per board applies its K slots' evaluations and
selects up to K new leaves under virtual loss), on the GPU box.

At 8x8 on boards 20 plies into random games, T = 4,096 node slots a board, the
uniform evaluator as integer tensors fixed on the device (priors 4,096
everywhere, values 0) and no observation, so the time is the library's alone:

  launch   E in {64, 1,024, 65,536} x K in {1, 4, 8, 16}: microseconds per
           advance_batch launch over a window of 24 launches from begin (at K = 16
           a longer one would fill the tree), between device events, the median of
           `reps` windows; the plain oth_puct_advance
           over the same window in the same run, alternating with it, as the
           yardstick; the mean number of leaves a launch emits per searched
           board and how often a board closed before its K-th slot (both from an
           untimed pass that reads the kinds back).
  split    how a launch divides between apply and select: after 16 launches, one
           launch with sim_limit = 0 (the K applies, no selection) against one
           full launch from the same state, and a launch on boards without leaves.
  search   the wall time of one 256-simulation puct_search whose evaluator is a
           small torch network (three 3x3 convolutions of 32 channels, a policy
           and a value head, random weights made here), through puct_quantize,
           for E in {64, 1,024} and K in {1, 8}: where K-fold fewer network calls
           show, or do not.

    python tools/probe_puct_batch.py [--out profiles/puct_batch.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, KS = (64, 1024, 65536), (1, 4, 8, 16)
N, T, PLIES, WINDOW, SIMS = 8, 4096, 20, 24, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "puct_batch.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import VecOthelloEnv
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def window(body, before, count):
        """us per call of `count` calls of body after `before` (untimed)."""
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(count):
            body()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / count

    def stats(xs):
        return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}

    out = {"launch": [], "split": [], "search": []}
    for E in a.sizes:
        env = VecOthelloEnv(E, board_size=N, seed=1, device=dev)
        env.step_policy("random", n_plies=PLIES, record=False)
        live = int((~env.terminated()).sum())
        pri1 = torch.full((E, N * N), 4096, dtype=torch.int32, device=dev)
        val1 = torch.zeros(E, dtype=torch.int32, device=dev)
        for K in a.ks:
            pri = torch.full((E * K, N * N), 4096, dtype=torch.int32, device=dev)
            val = torch.zeros(E * K, dtype=torch.int32, device=dev)
            plain_begin = lambda: env.puct_begin(max_tree_nodes=T, layout=None)  # noqa: E731
            plain = lambda: env.puct_advance(pri1, val1)  # noqa: E731
            batch_begin = lambda: env.puct_begin_batch(K, max_tree_nodes=T, layout=None)  # noqa: E731
            batch = lambda: env.puct_advance_batch(pri, val)  # noqa: E731
            tp, tb = [], []
            for r in range(a.reps + 1):  # alternating; the first round warms up
                p, b = window(plain, plain_begin, WINDOW), window(batch, batch_begin, WINDOW)
                if r:
                    tp.append(p)
                    tb.append(b)
            # the untimed pass: what a launch emits
            leaves = batch_begin()
            st = env.puct_result(status=True)[1]
            done = int((st == 0).sum())
            emitted, short = 0, 0
            for i in range(WINDOW):
                leaves = batch()
                per_board = (leaves.kind.view(E, K) != 0).sum(1)[st == 0]
                emitted += int(per_board.sum())
                if i:  # (the launch after begin applies the root alone: its batch is whole)
                    short += int((per_board < K).sum())
            vis = env.puct_result()
            sims = int(vis.sum()) // max(done, 1) + 1
            row = {"boards": E, "K": K, "searched_boards": done, "live_boards": live, "window": WINDOW,
                   "advance_batch_us": stats(tb), "advance_us": stats(tp),
                   "leaves_per_launch_per_board": emitted / float(WINDOW * max(done, 1)),
                   "boards_closed_early": short / float((WINDOW - 1) * max(done, 1)),
                   "simulations_after_window_mean": sims}
            row["us_per_leaf"] = row["advance_batch_us"]["median"] / max(row["leaves_per_launch_per_board"] * done, 1)
            row["advance_us_per_leaf"] = row["advance_us"]["median"] / max(done, 1)
            print(json.dumps(row), flush=True)
            out["launch"].append(row)

            # the apply / select split: single launches from the state after 16 launches
            def prepared():
                batch_begin()
                for _ in range(16):
                    batch()

            full, apply_only, idle = [], [], []
            for r in range(a.reps + 1):
                f = window(batch, prepared, 1)
                ao = window(lambda: env.puct_advance_batch(pri, val, sim_limit=0), prepared, 1)
                idl = window(lambda: env.puct_advance_batch(pri, val, sim_limit=0), lambda: None, 1)  # no leaf left
                if r:
                    full.append(f)
                    apply_only.append(ao)
                    idle.append(idl)
            row = {"boards": E, "K": K, "full_launch_us": stats(full), "apply_only_us": stats(apply_only),
                   "no_leaf_launch_us": stats(idle)}
            print(json.dumps(row), flush=True)
            out["split"].append(row)
            del pri, val
        env.close()
        env = None
        torch.cuda.empty_cache()

    # the end-to-end figure: a small network as the evaluator
    torch.manual_seed(0)
    body = torch.nn.Sequential(torch.nn.Conv2d(4, 32, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.ReLU()).to(dev)
    policy_head = torch.nn.Conv2d(32, 1, 1).to(dev)
    value_head = torch.nn.Linear(32, 1).to(dev)
    calls = [0]

    @torch.no_grad()
    def net(leaves):
        calls[0] += 1
        x = body(leaves.obs)
        return policy_head(x).flatten(1), torch.tanh(value_head(x.mean((2, 3))))[:, 0]

    for E in (64, 1024):
        if E not in a.sizes:
            continue
        env = VecOthelloEnv(E, board_size=N, seed=1, device=dev)
        env.step_policy("random", n_plies=PLIES, record=False)
        for K in (1, 8):
            wall, ncalls = [], 0
            for r in range(4):  # the first search warms up
                calls[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kw = dict(leaves_per_board=K) if K > 1 else {}
                vis = env.puct_search(net, SIMS, max_tree_nodes=T, **kw)
                torch.cuda.synchronize()
                if r:
                    wall.append((time.perf_counter() - t0) * 1e3)
                ncalls = calls[0]
            row = {"boards": E, "K": K, "simulations": SIMS, "search_wall_ms": stats(wall), "network_calls": ncalls,
                   "root_visits_max": int(vis.sum(1).max()) + 1}
            print(json.dumps(row), flush=True)
            out["search"].append(row)
        env.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "mapping": "one lane per board",
                   "board_size": N, "max_tree_nodes": T, "plies": PLIES, **out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
