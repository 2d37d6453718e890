#!/usr/bin/env python3
"""The cost of the self-play calls on the search's tree (oth_puct_pick and
oth_puct_reroot) beside the search of one move, on the GPU box.

Positions and search as tools/probe_puct.py: 8x8 boards 20 plies into random
games, 256 simulations of the uniform evaluator as integer tensors fixed on the
device (priors 4,096 everywhere, values 0), no observation, T = 1,024 and 4,096
node slots a board, E = 1,024, 8,192 and 65,536 boards.  In one run, as the
median over `reps` repetitions between device events after a warm-up:

  advances   the 256 puct_advance calls of one move (each repetition begins again)
  pick       one puct_pick with every board sampling
  reroot     one puct_reroot after step(best), in both mappings of the sweep: the
             shipped library (classify, a wave per board, finish) and the second
             library with the whole call on one lane a board
             (gymothelloenv_amd/variants/liboth_reroot_lane.so, built by
             __graft_entry__.build()); the workspace of the finished search is
             restored from a copy before every repetition, outside the timed
             window, and both mappings must leave the same leaves and results

and what the re-root saves: the share of boards kept and the mean visits a kept
root brings along (its children's visits; its own v is one more).

    python tools/probe_puct_play.py [--out profiles/puct_play.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1024, 8192, 65536)
TREES = (1024, 4096)
N, SIMS, PLIES = 8, 256, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "puct_play.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--trees", type=int, nargs="*", default=list(TREES))
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import VecOthelloEnv
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd import build as hb
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    if hb.needs_build(hb.REROOT_LANE_OUT, hb.REROOT_LANE_FLAGS):
        raise SystemExit("build the one-lane library first: python -c 'import __graft_entry__ as g; g.build()'")
    lane = L.load_path(hb.REROOT_LANE_OUT)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(body, before=None):
        """ms of one `body`: (median, min, max) over the repetitions."""
        out = []
        for _ in range(a.reps + 1):  # the first repetition warms up
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            body()
            e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        out = out[1:]
        return {"median": statistics.median(out), "min": min(out), "max": max(out)}

    res = []
    for E in a.sizes:
        for T in a.trees:
            env = VecOthelloEnv(E, board_size=N, seed=1, device=dev)
            other = VecOthelloEnv(E, board_size=N, seed=1, device=dev, lib=lane)
            env.step_policy("random", n_plies=PLIES, record=False)
            priors = torch.full((E, N * N), 4096, dtype=torch.int32, device=dev)
            values = torch.zeros(E, dtype=torch.int32, device=dev)
            row = {"boards": E, "board_size": N, "max_tree_nodes": T, "simulations": SIMS,
                   "live_boards": int((~env.terminated()).sum())}

            def search():
                for i in range(SIMS):
                    env.puct_advance(priors, values, more=i < SIMS - 1)

            row["advances_ms"] = timed(search, before=lambda: env.puct_begin(max_tree_nodes=T, layout=None))
            vis, nodes, st = env.puct_result(tree_nodes=True, status=True)
            row["tree_nodes_mean"] = float(nodes[st == 0].float().mean())
            row["pick_ms"] = timed(lambda: env.puct_pick(True, counter=0))
            actions = env.puct_pick()
            env.step(actions, observe=False)
            other.set_state(*env.get_state())
            other._puct_ws, other._puct = env._puct_ws, env._puct  # the same search, through the other library
            snap = env._puct_ws.clone()
            restore = lambda: env._puct_ws.copy_(snap)  # noqa: E731
            outs = {}
            for name, ev in (("wave", env), ("lane", other)):
                row["reroot_%s_ms" % name] = timed(lambda: ev.puct_reroot(actions), before=restore)
                restore()
                leaves, kept = ev.puct_reroot(actions, kept=True)
                outs[name] = [t.clone() for t in leaves[:4]] + [kept] + list(ev.puct_result(tree_nodes=True))
            for x, y in zip(outs["wave"], outs["lane"]):
                assert torch.equal(x, y), "the two mappings differ"
            kept, vis2, nodes2 = outs["wave"][4].bool(), outs["wave"][5], outs["wave"][6]
            row["kept_share"] = float(kept.float().mean())
            row["kept_root_child_visits_mean"] = float(vis2.sum(1)[kept].float().mean())
            row["kept_tree_nodes_mean"] = float(nodes2[kept].float().mean())
            row["reroot_wave_over_advances"] = row["reroot_wave_ms"]["median"] / row["advances_ms"]["median"]
            row["lane_over_wave"] = row["reroot_lane_ms"]["median"] / row["reroot_wave_ms"]["median"]
            print(json.dumps(row), flush=True)
            res.append(row)
            other._puct_ws = other._puct = None
            env.close()
            other.close()
            env = other = snap = None
            torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
