#!/usr/bin/env python3
"""The cost of the int8 network on the GPU box, beside the torch round trip it
replaces.

8x8 boards, two hidden layers.  Medians over `reps` repetitions after two
warm-ups, the versions of a row alternating:

  (a) eval    oth_net_eval (DeviceNet.evaluate) on R rows, between device events,
              against MLPPolicyValue of the same shape in torch (float32 and
              bfloat16) on net_features plus puct_quantize: what a simulation
              spends between two advances either way.  H = 256 over every R,
              H = 64 and 512 beside it.
  (b) search  wall time of a 256-simulation puct_search at 64 and 1,024 boards,
              K = 1 and 8 leaves a board, with a DeviceNet and with the float32
              torch module of the same shape; K = 1 also as one captured graph
              of (DeviceNet, advance) replayed.
  (c) split   oth_net_eval cut short after layer 0, after the hidden layers and
              after the head's logits (build.build_net_stop's variants), at R =
              1,024 and 65,536: where the kernel's time goes.

The variants are built where the main build's objects are:
    python tools/probe_net.py --build-variants
    python tools/probe_net.py [--out profiles/net.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, LAYERS = 8, 2
ROWS = (64, 512, 1024, 8192, 65536, 524288)
SIDE_ROWS = (64, 1024, 65536)  # H = 64 and 512
SEARCH = ((64, 1), (64, 8), (1024, 1), (1024, 8))
SIMS = 256
STAGES = ((1, "layer0"), (2, "hidden"), (3, "head"))


def mfma_per_tile(n, layers, H):
    """v_mfma_i32_16x16x64_i8 a tile of 16 rows: layer 0, the later layers, the head."""
    nn, W = n * n, (n * n + 63) // 64
    return {"layer0": (H // 16) * 3 * W, "hidden": (layers - 1) * (H // 16) * (H // 64),
            "head": ((nn + 1 + 15) // 16) * (H // 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--build-variants", action="store_true")
    a = ap.parse_args()
    from gymothelloenv_amd import build as hb
    if a.build_variants:
        for stage, _ in STAGES:
            print(hb.build_net_stop(stage))
        return
    import torch

    from gymothelloenv_amd import DeviceNet, MLPPolicyValue, VecOthelloEnv, net_features, puct_quantize
    from gymothelloenv_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(bodies, wall=False, reps=a.reps):
        """ms of each body, alternating them: {name: median / min / max} over the repetitions."""
        out = {k: [] for k in bodies}
        for rep in range(reps + 2):  # the first two repetitions warm up
            for k, body in bodies.items():
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

    def module_of(H):
        torch.manual_seed(0)
        return MLPPolicyValue(N, H, LAYERS).to(dev)

    def positions(R):
        env = VecOthelloEnv(min(R, 65536), board_size=N, auto_reset=True, seed=2, device=dev)
        env.reset()
        env.step_policy("random", 20, record=False)
        b, m, lg = env.get_state()
        env.close()
        k = (R + b.shape[0] - 1) // b.shape[0]
        return b.repeat(k, 1)[:R].contiguous(), m.repeat(k)[:R].contiguous(), lg.repeat(k, 1)[:R].contiguous()

    res = {"board_size": N, "layers": LAYERS, "reps": a.reps, "simulations": SIMS, "eval": [], "search": [],
           "split": [], "mfma_per_tile": {str(H): mfma_per_tile(N, LAYERS, H) for H in (64, 256, 512)}}
    for H, rows in ((256, ROWS), (64, SIDE_ROWS), (512, SIDE_ROWS)):
        module = module_of(H)
        half = module_of(H).to(torch.bfloat16)
        net = DeviceNet.from_module(module, device=dev)
        for R in rows:
            b, m, lg = positions(R)

            def torch_trip(mod, dtype):
                with torch.no_grad():
                    logits, values = mod(net_features(b, m, lg, N).to(dtype))
                return puct_quantize(logits, lg, values)

            t = timed({"net": lambda: net.evaluate(b, m, lg), "torch_f32": lambda: torch_trip(module, torch.float32),
                       "torch_bf16": lambda: torch_trip(half, torch.bfloat16)})
            res["eval"].append({"H": H, "rows": R, "net_ms": t["net"], "torch_f32_ms": t["torch_f32"],
                                "torch_bf16_ms": t["torch_bf16"],
                                "torch_f32_over_net": t["torch_f32"]["median"] / t["net"]["median"],
                                "torch_bf16_over_net": t["torch_bf16"]["median"] / t["net"]["median"]})
            print(res["eval"][-1], flush=True)
    # (b) a whole search
    module = module_of(256)
    net = DeviceNet.from_module(module, device=dev)
    float_eval = module.evaluator()
    for E, K in SEARCH:
        env = VecOthelloEnv(E, board_size=N, seed=3, device=dev)
        env.reset()
        env.step_policy("random", 12, record=False)
        kw = dict(layout=None, leaves_per_board=K)
        bodies = {"net": lambda: env.puct_search(net, SIMS, **kw), "torch_f32": lambda: env.puct_search(float_eval, SIMS, **kw)}
        row = {"boards": E, "K": K}
        if K == 1:
            T = min(max(64, SIMS * 60 // 4 + 64), L.OTH_PUCT_MAX_TREE_NODES)
            want = env.puct_search(net, SIMS, layout=None, max_tree_nodes=T).clone()
            leaves = env.puct_begin(layout=None, max_tree_nodes=T)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                env.puct_advance(*net(leaves))

            def graphed():
                fresh = env.puct_begin(layout=None, max_tree_nodes=T)  # (new tensors: the graph feeds on the old)
                for old, new in zip(leaves[:4], fresh[:4]):
                    old.copy_(new)
                for _ in range(SIMS - 1):
                    g.replay()
                env.puct_advance(*net(leaves), more=False)
                return env.puct_result()

            assert torch.equal(graphed(), want), "the replayed graph is not the eager search"
            bodies["net_graph"] = graphed
        t = timed(bodies, wall=True)
        row.update({k + "_wall_ms": v for k, v in t.items()})
        row["torch_f32_over_net"] = t["torch_f32"]["median"] / t["net"]["median"]
        res["search"].append(row)
        print(row, flush=True)
        env.close()
    # (c) the kernel's split, from the variants that stop early
    libs = {}
    for stage, name in STAGES:
        path = hb.net_stop_out(stage)
        if os.path.exists(path):
            libs[name] = L.load_path(path)
    if len(libs) == len(STAGES):
        for R in (1024, 65536):
            b, m, lg = positions(R)
            priors = torch.empty(R, N * N, dtype=torch.int32, device=dev)
            values = torch.empty(R, dtype=torch.int32, device=dev)

            def call(lib):
                def body():
                    L.check(lib.oth_net_eval(N, R, ctypes.byref(net.params), ctypes.c_void_p(net.blob.data_ptr()),
                                             net.blob.numel(), ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(m.data_ptr()),
                                             ctypes.c_void_p(lg.data_ptr()), ctypes.c_void_p(priors.data_ptr()),
                                             ctypes.c_void_p(values.data_ptr()), None,
                                             ctypes.c_void_p(stream.cuda_stream)), "oth_net_eval", lib)
                return body

            bodies = {name: call(lib) for name, lib in libs.items()}
            bodies["whole"] = call(L.load())
            t = timed(bodies)
            res["split"].append({"H": 256, "rows": R, "until_ms": t})
            print(res["split"][-1], flush=True)
    else:
        res["split_note"] = "the early-stop variants were not built (python tools/probe_net.py --build-variants)"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged.update(res)  # (the "convert" entry is tests/test_net_convert_cpu.py's and is kept)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
