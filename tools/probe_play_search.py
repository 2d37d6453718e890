#!/usr/bin/env python
"""oth_play_search on the GPU box: the per-call time of the fused self-play call
beside the unfused composition it replaces.

65,536 random-play 8x8 boards with exactly 30 empty squares (probe_search.py's
positions), the default weights on both colours, depths 1-4, n_plies 1 and 10:
  fused     one oth_play_search(n_plies) launch;
  unfused   n_plies x (oth_search's `best` + oth_step), the entry points the
            parent commit already had (search_actions + step).
Every repetition starts from the same boards (set_state outside the timed
region).  Recorded, not asserted: milliseconds per call (median, min, max over
the repetitions) and the share of fused plies played by the greedy fallback.

    python tools/probe_play_search.py [--out profiles/play_search/probe.json] [--reps 5]
        [--lib another_build.so]

--lib times another build of the library (an A/B arm) in place of the shipped one.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8
BOARDS = 65536
EMPTIES = 30
DEPTHS = (1, 2, 3, 4)
PLIES = (1, 10)


def timed(torch, stream, prepare, fn, reps):
    times = []
    for _ in range(reps):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "play_search", "probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", help="another build of the library (an A/B variant)")
    a = ap.parse_args()
    import torch
    from gymothelloenv_amd import SearchConfig, VecOthelloEnv, _lib
    lib = _lib.load_path(a.lib) if a.lib else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    env = VecOthelloEnv(BOARDS, board_size=N, seed=EMPTIES, device=dev, lib=lib)
    env.reset()
    env.step_policy("random", n_plies=N * N - 4 - EMPTIES, record=False)  # a ply places a disc
    b, m, lg = env.get_state()
    live = torch.nonzero((m & 2) == 0).flatten()
    pick = live[torch.arange(BOARDS, device=dev) % live.numel()]  # games that ended early: a live board's copy
    b, m, lg = b[pick].clone(), m[pick].clone(), lg[pick].clone()
    env.set_state(b, m, lg)
    assert bool((env.count_disks().sum(1) == N * N - EMPTIES).all())
    rows = []
    for depth in DEPTHS:
        cfg = SearchConfig(depth=depth)
        for plies in PLIES:
            def restore():
                env.set_state(b, m, lg)

            def fused():
                env.play_search(cfg, None, plies, record=True, fallbacks=True)

            def unfused():
                for _ in range(plies):
                    env.step(env.search_actions(depth=depth), observe=False)

            restore()
            fb = env.play_search(cfg, None, plies, fallbacks=True)[3]  # warm-up, and the fallbacks
            after_fused = [t.clone() for t in env.get_state()]
            restore()
            unfused()  # warm-up, and the same boards: both play the search's best move
            same = all(torch.equal(x, y) for x, y in zip(after_fused, env.get_state()))
            row = {"boards": BOARDS, "board_size": N, "empties": EMPTIES, "depth": depth, "n_plies": plies,
                   "fused_call_ms": timed(torch, stream, restore, fused, a.reps),
                   "unfused_call_ms": timed(torch, stream, restore, unfused, a.reps),
                   "fallback_share": float(fb.float().mean()), "same_final_boards": bool(same)}
            row["fused_over_unfused"] = row["fused_call_ms"]["median"] / row["unfused_call_ms"]["median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "lib": a.lib or "shipped", "rows": rows}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
