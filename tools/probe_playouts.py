#!/usr/bin/env python3
"""oth_playouts against what a user had to do without it, on the GPU box:

  call        VecOthelloEnv.playouts(R[, per_move=True])
  workaround  get_state; the rows replicated into a second handle of E*R boards
              (per move: E*N*N*R, a board for every square, legal or not);
              set_state there; per move one step() with each row's square;
              step_policy("random", N*N, record=False); the metas read back and
              reduced with torch

for three shapes from positions 20 plies into random 8x8 games: 65,536 boards at
R = 8 per board, 1,024 boards at R = 64 per move, one board at R = 65,536.  The
workaround uses nothing newer than get_state / set_state / step / step_policy.
Its second handle is keyed so that it plays the very games of the call (seed,
env ids and ply counter lined up with the call's id and counter formulas), so
the two results are compared as well, and the playout plies are counted once
from its final boards.  Times are medians over bursts between device events,
after a warm-up of both sides.

    python tools/probe_playouts.py [--out profiles/playouts.json] [--lib another_build.so]

--lib times another build of the library (an A/B arm, e.g. the playout unit under
other scheduler flags: profiles/playouts_sched_ab.json) in place of the shipped one.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((65536, 8, False), (1024, 64, True), (1, 65536, False))
SEED, COUNTER, N = 2024, 5, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playouts.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=4)
    ap.add_argument("--lib", help="another build of the library (an A/B variant) for both sides")
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import VecOthelloEnv, _lib
    lib = _lib.load_path(a.lib) if a.lib else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    nn = N * N

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
    for E, R, per_move in SHAPES:
        base = 1000
        env = VecOthelloEnv(E, board_size=N, seed=1, env_id_base=base, device=dev, lib=lib)
        env.step_policy("random", n_plies=20, record=False)
        S = nn * R if per_move else R
        # board j = e * S + a * R + r of the second handle gets the id of the call's playout (e, a, r)
        env2 = VecOthelloEnv(E * S, board_size=N, sudden_death_on_invalid_move=False, seed=SEED,
                             env_id_base=(base * S) % 2 ** 32, device=dev, lib=lib)
        squares = torch.arange(nn, dtype=torch.int32, device=dev).repeat_interleave(R).repeat(E)
        legal = env.legal_actions() & ~env.terminated()[:, None]

        def workaround():
            b, m, lg = env.get_state()
            env2.set_state(b.repeat_interleave(S, 0), m.repeat_interleave(S, 0), lg.repeat_interleave(S, 0))
            if per_move:
                env2.step(squares, observe=False)
            env2.ply_counter = COUNTER * 256
            env2.step_policy("random", n_plies=nn, record=False)
            _, m2, _ = env2.get_state()
            code = (m2.to(torch.int32) >> 2) & 3  # 0 draw, 1 white, 2 black
            white = (m.to(torch.int32) & 1).repeat_interleave(S, 0) != 0
            mine = torch.where(white, 1, 2)
            wdl = torch.stack([code == mine, code == 0, (code != mine) & (code != 0)], -1).to(torch.int32)
            wdl = wdl.view(E, S // R, R, 3).sum(2)
            if per_move:
                return wdl * legal[:, :, None]
            return wdl[:, 0] * (~env.terminated())[:, None]

        def call():
            return env.playouts(R, per_move=per_move, seed=SEED, id_key=0, counter=COUNTER)

        want, got = workaround(), call()  # warm-up of both sides, and the comparison
        same = bool(torch.equal(want, got))
        # plies = discs placed (per move: the root move too), from the workaround's final boards
        live = (legal if per_move else ~env.terminated()[:, None])
        discs0 = env.count_disks().sum(1)
        final = env2.count_disks().sum(1).view(E, S // R, R)
        plies = int(((final - discs0[:, None, None]) * live[:, :, None]).sum())
        playouts = int(live.sum()) * R
        tw, tc = timed(workaround), timed(call)
        row = {"boards": E, "n_playouts": R, "mode": "moves" if per_move else "root", "board_size": N,
               "playouts": playouts, "playout_plies": plies, "results_equal": same,
               "workaround_us": {"median": tw[0], "min": tw[1], "max": tw[2]},
               "call_us": {"median": tc[0], "min": tc[1], "max": tc[2]},
               "workaround_plies_per_s": plies / (tw[0] * 1e-6), "call_plies_per_s": plies / (tc[0] * 1e-6),
               "speedup": tw[0] / tc[0], "workaround_boards": E * S,
               "mean_legal_moves": float(legal.sum()) / max(1, int((~env.terminated()).sum()))}
        print(json.dumps(row), flush=True)
        res.append(row)
        env.close()
        env2.close()
        del env2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "burst": a.burst, "shapes": res}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
