#!/usr/bin/env python
"""The n-tuple network on the GPU box.

Rows: oth_ntuple_eval and oth_ntuple_update at 1,024 and 65,536 rows of 8x8 boards
(random play, 30 empty squares) with 12 snake tuples of length 8, beside a torch-only
composition of the same integers on the same device -- index arithmetic on the
bitboards, `gather`, `index_add_` -- whose results are compared with the library's
before anything is timed.  A timing is `calls` calls between two device events after a
warm-up, divided by `calls` -- the host's enqueue of a call lies inside the window, so at
1,024 rows the figure is what a loop of calls costs, not the kernel's time; the median of
`reps` such windows, with min and max.  The update's rate is fixed so that nearly every
row has a non-zero delta (the share is recorded).

Search: oth_search_ntuple at depths 1-4 on the boards tools/probe_search.py uses
(65,536 random-play 8x8 boards with exactly 30 and with 20 empty squares), beside
oth_search with the default weights on the same boards: milliseconds a call, nodes,
nodes per second.  The two searches place different numbers of discs (another
evaluation prunes differently), so the node rate is the comparison.

    python tools/probe_ntuple.py [--out profiles/ntuple/probe.json] [--reps 5] [--skip-rows] [--skip-search]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8
ROWS = (1024, 65536)
TUPLES, LENGTH, VALUE_SHIFT = 12, 8, 6
RATE, RATE_SHIFT = 1 << 12, 16  # a delta is a sixteenth of the error: nearly every row adds something
BOARDS = 65536
EMPTIES = (30, 20)
DEPTHS = (1, 2, 3, 4)


def timed(torch, stream, fn, calls, reps):
    """Milliseconds a call: `calls` calls between two events, `reps` windows."""
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / calls)
    return {"median": statistics.median(times), "min": min(times), "max": max(times), "calls": calls}


def positions(torch, E, empties, dev):
    """E live boards with `empties` empty squares from random play, as probe_search.py makes them."""
    from gymothelloenv_amd import VecOthelloEnv
    env = VecOthelloEnv(E, board_size=N, seed=empties, device=dev)
    env.reset()
    env.step_policy("random", n_plies=N * N - 4 - empties, record=False)
    b, m, lg = env.get_state()
    live = torch.nonzero((m & 2) == 0).flatten()
    pick = live[torch.arange(E, device=dev) % live.numel()]
    env.set_state(b[pick], m[pick], lg[pick])
    return env


def sigma(n, s, a):
    """The board symmetry s of square a (the header's words on oth_replay_gather)."""
    r, c = divmod(a, n)
    r, c = (c, r) if s & 1 else (r, c)
    return (n - 1 - r if s & 2 else r) * n + (n - 1 - c if s & 4 else c)


class TorchNet(object):
    """The same integers in torch alone: the tuples' transformed squares as an index tensor."""

    def __init__(self, torch, net):
        n, tp = net.board_size, net.tuples
        T = len(tp)
        sq = torch.zeros(T, 8, LENGTH, dtype=torch.int64)
        for t, squares in enumerate(tp):
            for s in range(8):
                for i, q in enumerate(squares):
                    sq[t, s, i] = sigma(n, s, q)
        self.torch, self.net = torch, net
        self.sq = sq.to(net.device)  # (T, 8, L)
        self.pow3 = (3 ** torch.arange(LENGTH, dtype=torch.int64)).to(net.device)
        self.off = torch.tensor(net.offsets, dtype=torch.int64, device=net.device)

    def entries(self, boards, meta):
        torch = self.torch
        R = meta.numel()
        white = (meta.to(torch.int64) & 1).bool()[:, None]
        M = torch.where(white, boards[:, 1:2], boards[:, 0:1])
        O = torch.where(white, boards[:, 0:1], boards[:, 1:2])
        sq = self.sq.reshape(1, -1)
        m, o = (M >> sq) & 1, (O >> sq) & 1  # (R, T 8 L)
        cell = (m | ((o & ~m) << 1)).reshape(R, -1, 8, LENGTH)
        return (cell * self.pow3).sum(3) + self.off[None, :, None]  # (R, T, 8)

    def evaluate(self, boards, meta, weights):
        torch = self.torch
        e = self.entries(boards, meta).reshape(meta.numel(), -1)
        sums = weights[-1].to(torch.int64) + weights.to(torch.int64)[e].sum(1)
        return torch.clamp(sums >> VALUE_SHIFT, -32768, 32768).to(torch.int32), e

    def update(self, boards, meta, targets, weights, rate, rate_shift):
        torch = self.torch
        v, e = self.evaluate(boards, meta, weights)
        x = (torch.clamp(targets.to(torch.int64), -32768, 32768) - v) * rate
        x = (x + (1 << (rate_shift - 1))) >> rate_shift
        d = torch.clamp(x, -2 ** 30, 2 ** 30).to(torch.int32)
        weights.index_add_(0, e.reshape(-1), d[:, None].expand(-1, e.shape[1]).reshape(-1))
        weights[-1] += d.sum(dtype=torch.int32)
        return d


def rows_part(torch, a):
    from gymothelloenv_amd import NTupleNet, snake_tuples
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    net = NTupleNet(N, snake_tuples(N, TUPLES, LENGTH, seed=1), VALUE_SHIFT, device=dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    w0 = torch.randint(-20000, 20001, (net.weight_count,), generator=g, dtype=torch.int32).to(dev)
    tnet = TorchNet(torch, net)
    out = []
    for R in ROWS:
        env = positions(torch, R, 30, dev)
        boards, meta, _ = env.get_state()
        targets = torch.randint(-32768, 32769, (R,), generator=g, dtype=torch.int32).to(dev)
        rate, rate_shift = RATE, RATE_SHIFT
        # the same integers first
        net.weights.copy_(w0)
        wt = w0.clone()
        assert torch.equal(net.evaluate(boards, meta), tnet.evaluate(boards, meta, wt)[0])
        d = net.update(boards, meta, targets, rate, rate_shift)
        assert torch.equal(d, tnet.update(boards, meta, targets, wt, rate, rate_shift)) and torch.equal(net.weights, wt)
        calls = 200 if R <= 4096 else 20
        row = {"rows": R, "board_size": N, "tuples": TUPLES, "length": LENGTH, "weights": net.weight_count,
               "eval_ms": timed(torch, stream, lambda: net.evaluate(boards, meta), calls, a.reps),
               "update_ms": timed(torch, stream, lambda: net.update(boards, meta, targets, rate, rate_shift), calls, a.reps),
               "torch_eval_ms": timed(torch, stream, lambda: tnet.evaluate(boards, meta, wt), calls, a.reps),
               "torch_update_ms": timed(torch, stream, lambda: tnet.update(boards, meta, targets, wt, rate, rate_shift),
                                        calls, a.reps)}
        d = net.update(boards, meta, targets, rate, rate_shift)
        row["adding_rows_share"] = float((d != 0).float().mean())  # (a row with delta 0 adds nothing)
        row["gathers_per_s"] = R * 8 * TUPLES / (row["eval_ms"]["median"] * 1e-3)
        row["atomics_per_s"] = R * (8 * TUPLES + 1) / (row["update_ms"]["median"] * 1e-3)  # (a lower bound: the time holds the delta pass too)
        print(json.dumps(row), flush=True)
        out.append(row)
        env.close()
    return out


def search_part(torch, a):
    from gymothelloenv_amd import NTupleNet, snake_tuples
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    net = NTupleNet(N, snake_tuples(N, TUPLES, LENGTH, seed=1), VALUE_SHIFT, device=dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    net.weights.copy_(torch.randint(-20000, 20001, (net.weight_count,), generator=g, dtype=torch.int32))
    out = []
    for empties in EMPTIES:
        env = positions(torch, BOARDS, empties, dev)
        for depth in DEPTHS:
            row = {"boards": BOARDS, "board_size": N, "empties": empties, "depth": depth}
            for name, fn in (("ntuple", lambda: env.search_ntuple(depth, net, status=True, nodes=True)),
                             ("wpc", lambda: env.search(depth, status=True, nodes=True))):
                res = fn()  # warm-up, and the counts
                torch.cuda.synchronize()
                total = int(res[2].sum())
                ms = timed(torch, stream, fn, 1 if depth >= 3 else 10, a.reps)
                row[name] = {"call_ms": ms, "nodes": total, "nodes_per_s": total / (ms["median"] * 1e-3),
                             "aborted": int((res[1] == 4).sum())}
            row["node_rate_ratio"] = row["ntuple"]["nodes_per_s"] / row["wpc"]["nodes_per_s"]
            print(json.dumps(row), flush=True)
            out.append(row)
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntuple", "probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-rows", action="store_true")
    ap.add_argument("--skip-search", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    if not a.skip_rows:
        res["rows"] = rows_part(torch, a)
    if not a.skip_search:
        res["search"] = search_part(torch, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
