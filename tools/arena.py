#!/usr/bin/env python
"""The playing strength of SearchConfig(depth=k) with the default weights, on
the GPU box: win / draw / loss counts over 16,384 8x8 games per pairing and
colour, each game after up to 10 random opening plies (initial_rand_steps=10:
without them two deterministic movers play one game per colour), auto-reset
off.  The search is SearchConfig(depth=k, endgame_empties=10), k = 1..4.

  search against random / greedy / maximin3: the search is the embedded opponent
      of reset_vs / step_vs (oth_reset_vs_search / oth_step_vs_search), the
      scripted mover plays the protagonist's actions (policy_actions; a uniform
      pick of legal_actions for random); counts_vs is the scripted side's tally.
  search against search: play_search(black, white) until every game is over;
      counts is the tally by colour.
Both colours of every pairing.  Recorded, not asserted.

    python tools/arena.py [--out profiles/play_search/arena.json] [--games 16384]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8
DEPTHS = (1, 2, 3, 4)
SCRIPTED = ("random", "greedy", "maximin3")
OPENING_PLIES = 10
ENDGAME_EMPTIES = 10


def scripted_actions(torch, env, who, gen):
    if who != "random":
        return env.policy_actions(who)
    lb = env.legal_actions().float()
    lb[lb.sum(1) == 0, 0] = 1.0  # (a finished board: any square, the call ignores it)
    return torch.multinomial(lb, 1, generator=gen).flatten().to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "play_search", "arena.json"))
    ap.add_argument("--games", type=int, default=16384)
    a = ap.parse_args()
    import torch
    from gymothelloenv_amd import SearchConfig, VecOthelloEnv
    dev = torch.device("cuda", 0)
    G = a.games
    cfgs = {k: SearchConfig(depth=k, endgame_empties=ENDGAME_EMPTIES) for k in DEPTHS}
    rows = []
    for k in DEPTHS:
        for who in SCRIPTED:
            for colour, name in ((1, "black"), (-1, "white")):  # the search's colour; the scripted side is the protagonist
                t0 = time.time()
                gen = torch.Generator(device=dev).manual_seed(1000 * k + colour)
                env = VecOthelloEnv(G, board_size=N, seed=200 + k, initial_rand_steps=OPENING_PLIES, device=dev)
                prot = torch.full((G,), colour, dtype=torch.int8)
                env.reset_vs(cfgs[k], protagonist=prot)
                calls = fallbacks = 0
                while not bool(env.terminated().all()):
                    res = env.step_vs(scripted_actions(torch, env, who, gen), cfgs[k], observe=False, fallbacks=True)
                    fallbacks += int(res[4].sum())
                    calls += 1
                    assert calls <= N * N
                w, d, l = [int(x) for x in env.counts_vs().cpu()]
                assert w + d + l == G
                row = {"games": G, "board_size": N, "search_depth": k, "search_colour": name, "against": who,
                       "opening_plies": OPENING_PLIES, "endgame_empties": ENDGAME_EMPTIES, "wins": l, "draws": d,
                       "losses": w, "fallback_plies": fallbacks, "seconds": time.time() - t0}
                print(json.dumps(row), flush=True)
                rows.append(row)
                env.close()
    for k in DEPTHS:
        for j in DEPTHS:
            if j <= k:
                continue
            for black, white in ((k, j), (j, k)):
                t0 = time.time()
                env = VecOthelloEnv(G, board_size=N, seed=300 + 10 * k + j, initial_rand_steps=OPENING_PLIES,
                                    device=dev)
                env.reset()
                calls = 0
                while not bool(env.terminated().all()):
                    env.play_search(cfgs[black], cfgs[white], n_plies=10, record=False)
                    calls += 1
                    assert calls <= 2 * N * N
                bw, d, ww = [int(x) for x in env.counts().cpu()]
                assert bw + d + ww == G
                row = {"games": G, "board_size": N, "black_depth": black, "white_depth": white,
                       "opening_plies": OPENING_PLIES, "endgame_empties": ENDGAME_EMPTIES, "black_wins": bw,
                       "draws": d, "white_wins": ww, "seconds": time.time() - t0}
                print(json.dumps(row), flush=True)
                rows.append(row)
                env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
