#!/usr/bin/env python3
"""The cost of the root noise on the GPU box, beside the torch version it replaces.

8x8 boards.  Medians over `reps` repetitions after two warm-ups, the versions of a
row alternating:

  (a) call   oth_puct_noise (VecOthelloEnv.puct_noise, root mode, in place) on E rows
             of priors, between device events, against the same step in torch:
             torch.distributions.Dirichlet(alpha) sampled over N*N squares, masked to
             the legal ones and renormalised, mixed into the priors as floats and
             requantised to int32 -- what a caller without the call would write.
  (b) move   wall time of one 256-simulation puct_play move with a DeviceNet of two
             hidden layers of 256, with and without noise=RootNoise(...): the
             difference holds the two noise calls and the extra evaluation of the
             stepped position.

    python tools/probe_noise.py [--out profiles/noise.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, LAYERS, H = 8, 2, 256
CALL_BOARDS = (64, 1024, 65536)
MOVE_BOARDS = (64, 1024)
SIMS = 256
EPSILON, ALPHA = 0.25, 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--move-reps", type=int, default=7)
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import DeviceNet, MLPPolicyValue, RootNoise, VecOthelloEnv
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(bodies, wall=False, reps=a.reps, before=None):
        """ms of each body, alternating them: {name: median / min / max} over the repetitions."""
        out = {k: [] for k in bodies}
        for rep in range(reps + 2):  # the first two repetitions warm up
            for k, body in bodies.items():
                if before is not None:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                body()
                e1.record(stream)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if rep >= 2:
                    out[k].append((t1 - t0) * 1e3 if wall else e0.elapsed_time(e1))
        return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in out.items()}

    noise = RootNoise(EPSILON, ALPHA)
    table = noise.table_on(dev)
    torch.manual_seed(0)
    net = DeviceNet.from_module(MLPPolicyValue(N, H, LAYERS).to(dev), device=dev)
    res = {"board_size": N, "reps": a.reps, "move_reps": a.move_reps, "simulations": SIMS, "epsilon_256": noise.epsilon,
           "alpha": ALPHA, "net": {"layers": LAYERS, "width": H}, "call": [], "move": []}
    nn = N * N
    sq = torch.arange(nn, device=dev)
    for E in CALL_BOARDS:
        env = VecOthelloEnv(E, board_size=N, auto_reset=True, seed=2, device=dev)
        env.reset()
        env.step_policy("random", 20, record=False)
        boards, meta, legal = env.get_state()
        priors = net.evaluate(boards, meta, legal)[0]
        mask = ((legal[:, sq // 64] >> (sq % 64)) & 1).bool()
        dist = torch.distributions.Dirichlet(torch.full((nn,), ALPHA, device=dev))

        def in_torch():
            eta = dist.sample((E,)) * mask
            eta = eta / eta.sum(1, keepdim=True).clamp_min(1e-30)
            p = priors.to(torch.float32) * (1.0 - EPSILON) + eta * (EPSILON * 65535.0)
            return torch.where(mask, torch.round(p).to(torch.int32), priors)

        work = priors.clone()
        t = timed({"noise": lambda: env.puct_noise(work, noise.epsilon, table, out=work, counter=1),
                   "torch": in_torch})
        res["call"].append({"boards": E, "noise_ms": t["noise"], "torch_ms": t["torch"],
                            "torch_over_noise": t["torch"]["median"] / t["noise"]["median"]})
        print(res["call"][-1], flush=True)
        env.close()
    for E in MOVE_BOARDS:
        env = VecOthelloEnv(E, board_size=N, seed=3, device=dev)
        state = {}

        def fresh():
            """Every timed move starts from the same positions and a new search."""
            if not state:
                env.reset()
                env.step_policy("random", 12, record=False)
                state["s"] = [t.clone() for t in env.get_state()]
            env.set_state(*state["s"])
            env._puct = None

        t = timed({"plain": lambda: env.puct_play(net, SIMS, layout=None),
                   "noise": lambda: env.puct_play(net, SIMS, layout=None, noise=noise)}, wall=True, reps=a.move_reps,
                  before=fresh)
        res["move"].append({"boards": E, "plain_wall_ms": t["plain"], "noise_wall_ms": t["noise"],
                            "noise_minus_plain_ms": t["noise"]["median"] - t["plain"]["median"]})
        print(res["move"][-1], flush=True)
        env.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
