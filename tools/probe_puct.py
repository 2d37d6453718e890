#!/usr/bin/env python3
"""The cost of one simulation of the network-guided tree search (oth_puct_advance:
one lane per board applies the pending leaf's evaluation and descends to the
next leaf; a second launch writes the leaves' observation), on the GPU box.

At 8x8 for E = 1,024, 8,192 and 65,536 boards 20 plies into random games, with
T = 1,024 node slots a board and 256 simulations of the uniform evaluator as
integer tensors fixed on the device (priors 4,096 everywhere, values 0), so the
time is the library's alone:

  eager     256 puct_advance calls from Python (make_state float32 leaves), and
            the same without the observation (layout=None: one launch a call)
  graphed   one advance captured in a HIP graph, replayed 256 times

in microseconds per advance, the median over `reps` searches between device
events (each search begins again from the same boards, so every repetition does
the same work; the begin is outside the timed window).  Beside them, on the
same boards, the scale: observe(make_state, float32) alone and an empty-kernel
launch (a fill of one element), eager and graphed, 256 a window.

    python tools/probe_puct.py [--out profiles/puct.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1024, 8192, 65536)
N, T, SIMS, PLIES = 8, 1024, 256, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "puct.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--variant", default=None, help="NAME=PATH of another build of the library (build.build with "
                    "extra_flags and out=...): its advance without the observation against the shipped one, "
                    "alternating, three rounds")
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import VecOthelloEnv
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(body, before=None):
        """us per call of `body`'s SIMS calls: (median, min, max) over the repetitions."""
        out = []
        for _ in range(a.reps + 1):  # the first repetition warms up
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            for _ in range(SIMS):
                body()
            e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / SIMS)
        out = out[1:]
        return {"median": statistics.median(out), "min": min(out), "max": max(out)}

    def graph_of(fn):
        fn()  # warm
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    res = []
    for E in a.sizes:
        env = VecOthelloEnv(E, board_size=N, seed=1, device=dev)
        env.step_policy("random", n_plies=PLIES, record=False)
        priors = torch.full((E, N * N), 4096, dtype=torch.int32, device=dev)
        values = torch.zeros(E, dtype=torch.int32, device=dev)
        row = {"boards": E, "board_size": N, "max_tree_nodes": T, "simulations": SIMS,
               "live_boards": int((~env.terminated()).sum())}
        for name, layout in (("advance_make_state_f32", "make_state"), ("advance_no_obs", None)):
            begin = lambda: env.puct_begin(max_tree_nodes=T, layout=layout)  # noqa: E731
            adv = lambda: env.puct_advance(priors, values)  # noqa: E731
            begin()
            row[name + "_eager_us"] = timed(adv, before=begin)
            vis, nodes, st = env.puct_result(tree_nodes=True, status=True)
            assert int(vis.sum()) == int((st == 0).sum()) * (SIMS - 1)
            row["tree_nodes_mean"] = float(nodes[st == 0].float().mean())
            row["tree_nodes_max"] = int(nodes.max())
            begin()
            g = graph_of(adv)
            row[name + "_graphed_us"] = timed(g.replay, before=begin)
            del g
        obs = env.observe("make_state", torch.float32)
        ob = lambda: env.observe("make_state", torch.float32, out=obs)  # noqa: E731
        row["observe_make_state_f32_eager_us"] = timed(ob)
        g = graph_of(ob)
        row["observe_make_state_f32_graphed_us"] = timed(g.replay)
        one = torch.zeros(1, device=dev)
        fill = lambda: one.fill_(1.0)  # noqa: E731
        row["empty_launch_eager_us"] = timed(fill)
        g = graph_of(fill)
        row["empty_launch_graphed_us"] = timed(g.replay)
        del g
        if a.variant:
            from gymothelloenv_amd import _lib as L
            name, path = a.variant.split("=", 1)
            other = VecOthelloEnv(E, board_size=N, seed=1, device=dev, lib=L.load_path(path))
            other.step_policy("random", n_plies=PLIES, record=False)
            envs = (("shipped", env), (name, other))
            ab = dict((k, []) for k, _ in envs)
            for _ in range(3):
                for k, ev in envs:
                    begin = lambda: ev.puct_begin(max_tree_nodes=T, layout=None)  # noqa: E731
                    ab[k].append(timed(lambda: ev.puct_advance(priors, values), before=begin)["median"])
            assert torch.equal(env.puct_result(), other.puct_result())  # the same search
            row["ab_advance_no_obs_eager_us"] = ab
            other.close()
        print(json.dumps(row), flush=True)
        res.append(row)
        env.close()
        env = None
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "mapping": "one lane per board",
                   "rows": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
