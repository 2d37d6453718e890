#!/usr/bin/env python3
"""The cost of the replay store's calls on the GPU box, beside a torch-only
implementation of the same minibatch and beside one puct_advance.

8x8 boards.  A store of 65,536 rows (1,024 boards x 64 slots) and of 1,048,576
rows (16,384 x 64) is filled by 64 moves of append / random play with auto-reset
/ label and a last label of every board, so that every row is LABELLED.  In one
run, as the median over `reps` repetitions between device events after a
warm-up, alternating the two versions:

  sample        replay_sample(n, augment=True) with obs in make_state / float32,
                n = 1,024 and 4,096: the rank step's two launches, the batch
                kernel (a lane per sample) and the observation launch
  torch         the same batch from the same stored arrays (the store dumped once
                through replay_gather) with tensor ops alone: nonzero on the
                states, index selection of the drawn rows, a scatter of the
                visits and of the three bit planes with symmetry_permutations,
                and the four make_state planes built from them; its draw is
                torch.randint, and with the device's own rows and symmetries it
                must give the device's obs, visits and outcome bit for bit
  append+label  one replay_append and one replay_label per move at 1,024 and
                65,536 boards (horizon 64), against the 28-60 us of one
                puct_advance that DESIGN.md section 5 records

    python tools/probe_replay.py [--out profiles/replay.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H = 8, 64
STORES = (1024, 16384)  # boards: 65,536 and 1,048,576 rows
BATCHES = (1024, 4096)
MOVE_SIZES = (1024, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--stores", type=int, nargs="*", default=list(STORES))
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import VecOthelloEnv, symmetry_permutations
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    nn = N * N

    def timed(bodies):
        """ms of each body, alternating them: {name: (median, min, max)} over the repetitions."""
        out = {k: [] for k in bodies}
        for rep in range(a.reps + 2):  # the first two repetitions warm up
            for k, body in bodies.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(stream)
                body()
                e1.record(stream)
                torch.cuda.synchronize()
                if rep >= 2:
                    out[k].append(e0.elapsed_time(e1))
        return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in out.items()}

    def filled(E):
        env = VecOthelloEnv(E, board_size=N, auto_reset=True, seed=1, device=dev)
        env.replay_begin(H, 4096)
        ones = torch.ones(E, nn, dtype=torch.int32, device=dev)
        for _ in range(H):
            env.replay_append(ones)
            _, rewards, dones = env.step_policy("random", 1)
            env.replay_label(rewards[0], dones[0])
        env.replay_label(torch.zeros(E, dtype=torch.int32, device=dev), torch.ones(E, dtype=torch.uint8, device=dev))
        counts = env.replay_counts().tolist()
        assert counts == [0, 0, E * H], counts
        return env

    perms = symmetry_permutations(N).to(dev)
    sq = torch.arange(nn, device=dev)

    def planes_of(words):  # int64 (n, 1) -> bool (n, 64)
        return ((words >> sq) & 1).bool()

    res = {"board_size": N, "horizon": H, "reps": a.reps, "sample": [], "move": []}
    for E in a.stores:
        env = filled(E)
        R = E * H
        # the store as tensors, dumped once
        parts = [env.replay_gather(torch.arange(lo, min(lo + 4096, R), dtype=torch.int32, device=dev), layout=None)
                 for lo in range(0, R, 4096)]
        state, boards, meta, legal, visits, outcome = (torch.cat([getattr(p, k) for p in parts]) for k in
                                                       ("state", "boards", "meta", "legal", "visits", "outcome"))
        del parts

        def torch_batch(n, rows=None, sym=None):
            lab = torch.nonzero(state == 2).squeeze(1)
            if rows is None:
                rows = lab[torch.randint(lab.numel(), (n,), device=dev)]
                sym = torch.randint(8, (n,), device=dev)
            to = perms[sym.long()]  # (n, 64): sigma_s(a)
            b = boards[rows]
            black = torch.zeros(n, nn, dtype=torch.bool, device=dev).scatter_(1, to, planes_of(b[:, :1]))
            white = torch.zeros(n, nn, dtype=torch.bool, device=dev).scatter_(1, to, planes_of(b[:, 1:]))
            moves = torch.zeros(n, nn, dtype=torch.bool, device=dev).scatter_(1, to, planes_of(legal[rows]))
            turn = (meta[rows] & 1).bool()[:, None].expand(n, nn)
            moves = moves & (moves.sum(1, keepdim=True) >= 2)
            obs = torch.stack([black, white, turn, moves], dim=1).to(torch.float32).view(n, 4, N, N)
            vis = torch.zeros(n, nn, dtype=torch.int32, device=dev).scatter_(1, to, visits[rows])
            return obs, vis, outcome[rows]

        for n in BATCHES:
            got = env.replay_sample(n, seed=3, counter=1)
            obs, vis, out = torch_batch(n, got.rows.long(), got.sym)
            assert torch.equal(obs, got.obs) and torch.equal(vis, got.visits) and torch.equal(out, got.outcome)
            t = timed({"sample": lambda: env.replay_sample(n), "torch": lambda: torch_batch(n)})
            res["sample"].append({"rows": R, "n": n, "sample_ms": t["sample"], "torch_ms": t["torch"],
                                  "torch_over_sample": t["torch"]["median"] / t["sample"]["median"]})
            print(res["sample"][-1], flush=True)
        env.close()
        del state, boards, meta, legal, visits, outcome
    for E in MOVE_SIZES:
        env = VecOthelloEnv(E, board_size=N, auto_reset=True, seed=1, device=dev)
        env.replay_begin(H, 4096)
        ones = torch.ones(E, nn, dtype=torch.int32, device=dev)
        rewards = torch.zeros(E, dtype=torch.int32, device=dev)
        dones = (torch.arange(E, device=dev) % 60 == 0).to(torch.uint8)  # a game in sixty ends at a move

        def move():
            env.replay_append(ones)
            env.replay_label(rewards, dones)

        t = timed({"append_label": move, "append": lambda: env.replay_append(ones),
                   "label": lambda: env.replay_label(rewards, dones)})
        res["move"].append({"boards": E, "append_label_ms": t["append_label"], "append_ms": t["append"],
                            "label_ms": t["label"]})
        print(res["move"][-1], flush=True)
        env.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
