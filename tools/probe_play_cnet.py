#!/usr/bin/env python3
"""The cost of the conv net as a player on the GPU box, beside the composition it replaces.

8x8 boards, two DeviceConvNets (C = 64, B = 4 and C = 128, B = 8), E = 1,024 and
65,536 boards.  Medians over `reps` repetitions after two warm-ups, the versions of
a row alternating; every timed body starts from the same positions (ten random plies
from the reset boards) and runs between device events.

  play      VecOthelloEnv.play_net, 10 plies a launch, deterministic player: us a ply
  compose   the same ten plies from what the library had before: per ply get_state ->
            DeviceConvNet.evaluate(logits=True) -> torch argmax over the legal squares
            on the device -> step (no host step, no synchronise inside the window): the
            baseline, us a ply
  step_vs   one step_vs call against NetPlayer (the protagonist plays greedy_actions,
            computed outside the window), without the observation: us a call
  net_eval  DeviceConvNet.evaluate alone on E rows, the floor of a ply (the play kernel
            runs the same convs on a board a workgroup): us a call

    python tools/probe_play_cnet.py [--out profiles/play_cnet.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8
NETS = ((64, 4), (128, 8))  # (channels, blocks)
BOARDS = (1024, 65536)
PLIES = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "play_cnet.json"))
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import ConvPolicyValue, DeviceConvNet, NetPlayer, VecOthelloEnv
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(bodies, before, reps=a.reps):
        """ms of each body, alternating them: {name: median / min / max} over the repetitions."""
        out = {k: [] for k in bodies}
        for rep in range(reps + 2):  # the first two repetitions warm up
            for k, body in bodies.items():
                before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(stream)
                body()
                e1.record(stream)
                torch.cuda.synchronize()
                if rep >= 2:
                    out[k].append(e0.elapsed_time(e1))
        return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in out.items()}

    torch.manual_seed(0)
    nn = N * N
    sq = torch.arange(nn, device=dev)
    res = {"board_size": N, "reps": a.reps, "plies": PLIES, "rows": []}
    for C, B, E in [(C, B, E) for C, B in NETS for E in BOARDS]:
        net = DeviceConvNet.from_module(ConvPolicyValue(N, C, B).to(dev), device=dev)
        player = NetPlayer(net)
        env = VecOthelloEnv(E, board_size=N, sudden_death_on_invalid_move=False, seed=2, device=dev)
        env.reset()
        env.step_policy("random", 10, record=False)
        start = [t.clone() for t in env.get_state()]
        acts = torch.zeros(E, dtype=torch.int32, device=dev)
        prot = torch.where((start[1] & 1) != 0, 1, -1).to(torch.int8)  # the protagonist is the side to move

        def fresh():
            env.set_state(*start)
            acts.copy_(env.greedy_actions())

        def compose():
            for _ in range(PLIES):
                boards, meta, legal = env.get_state()
                z = net.evaluate(boards, meta, legal, logits=True)[2][:, :nn]
                mask = ((legal[:, sq // 64] >> (sq % 64)) & 1).bool()
                key = torch.where(mask, z.to(torch.int64), torch.full_like(z, -2 ** 40, dtype=torch.int64))
                a_ = torch.where(mask.any(1), key.argmax(1), torch.full((E,), -1, device=dev)).to(torch.int32)
                env.step(a_)

        # the two ways play the same moves from the same boards (argmax picks the first maximum: the lowest square)
        fresh()
        one = env.play_net(player, None, PLIES)[0]
        after_one = [t.clone() for t in env.get_state()]
        fresh()
        compose()
        same = all(torch.equal(x, y) for x, y in zip(after_one, env.get_state()))

        t = timed({"play": lambda: env.play_net(player, None, PLIES, record=False), "compose": compose,
                   "step_vs": lambda: env.step_vs(acts, player, protagonist=prot, observe=False),
                   "net_eval": lambda: net.evaluate(*start)}, fresh)
        row = {"channels": C, "blocks": B, "boards": E, "same_boards_after_both": bool(same), "moves_played": int((one >= 0).sum()),
               "play_us_per_ply": 1e3 * t["play"]["median"] / PLIES,
               "compose_us_per_ply": 1e3 * t["compose"]["median"] / PLIES,
               "step_vs_us_per_call": 1e3 * t["step_vs"]["median"], "net_eval_us": 1e3 * t["net_eval"]["median"],
               "compose_over_play": t["compose"]["median"] / t["play"]["median"], "ms": t}
        res["rows"].append(row)
        print({k: v for k, v in row.items() if k != "ms"}, flush=True)
        env.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
