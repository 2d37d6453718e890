#!/usr/bin/env python3
"""The cost of the int8 convolutional network on the GPU box, beside the torch
module it replaces and beside the int8 MLP.

8x8 boards, C = 64 / B = 4 and C = 128 / B = 8.  Medians over `reps` repetitions
after two warm-ups, the versions of a row alternating (the method of
tools/probe_net.py):

  (a) eval    oth_cnet_eval (DeviceConvNet.evaluate) on R = 1,024 and 65,536 rows,
              between device events, against ConvPolicyValue of the same shape in
              torch -- float32, and bfloat16 in channels-last -- on net_features
              plus puct_quantize, and against oth_net_eval (two layers of 256).
  (b) search  wall time of a 256-simulation puct_search at 64 and 1,024 boards with
              a DeviceConvNet and with the float32 torch module of the same shape.

The file is written after every row, so a run that is cut short leaves what it
measured.
    python tools/probe_cnet.py [--out profiles/cnet.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8
SHAPES = ((64, 4), (128, 8))
ROWS = (1024, 65536)
SEARCH_BOARDS = (64, 1024)
SIMS = 256


def mfma_per_row(n, C, B):
    """v_mfma_i32_16x16x64_i8 a row (board): the stem, the 2 B convs, the head; 16 x 16 x 64 MACs each."""
    st, ot, ks = (n * n + 15) // 16, C // 16, C // 64
    return {"stem": ot * st, "convs": 2 * B * ot * 9 * ks * st, "head": 9 * ks * st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnet.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--skip-search", action="store_true")
    a = ap.parse_args()
    import torch

    from gymothelloenv_amd import (ConvPolicyValue, DeviceConvNet, DeviceNet, MLPPolicyValue, VecOthelloEnv, net_features,
                                   puct_quantize)
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

    def positions(R):
        env = VecOthelloEnv(min(R, 65536), board_size=N, auto_reset=True, seed=2, device=dev)
        env.reset()
        env.step_policy("random", 20, record=False)
        b, m, lg = env.get_state()
        env.close()
        k = (R + b.shape[0] - 1) // b.shape[0]
        return b.repeat(k, 1)[:R].contiguous(), m.repeat(k)[:R].contiguous(), lg.repeat(k, 1)[:R].contiguous()

    res = {"board_size": N, "reps": a.reps, "simulations": SIMS, "eval": [], "search": [],
           "mfma_per_row": {"C%d_B%d" % s: mfma_per_row(N, *s) for s in SHAPES}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged.update(res)  # (the "convert" entry is tests/test_cnet_convert_cpu.py's and is kept)
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)
            f.write("\n")

    torch.manual_seed(0)
    mlp = DeviceNet.from_module(MLPPolicyValue(N, 256, 2).to(dev), device=dev)
    modules = {}
    for C, B in SHAPES:
        torch.manual_seed(0)
        module = ConvPolicyValue(N, C, B).to(dev)
        half = ConvPolicyValue(N, C, B).to(dev)
        half.load_state_dict(module.state_dict())
        half = half.to(torch.bfloat16).to(memory_format=torch.channels_last)
        modules[(C, B)] = (module, half, DeviceConvNet.from_module(module, device=dev))
    for R in ROWS:
        b, m, lg = positions(R)
        for (C, B), (module, half, net) in modules.items():
            def torch_trip(mod, dtype, last):
                with torch.no_grad():
                    x = net_features(b, m, lg, N).to(dtype).reshape(-1, 3, N, N)
                    if last:
                        x = x.contiguous(memory_format=torch.channels_last)
                    logits, values = mod(x)
                return puct_quantize(logits.float(), lg, values.float())

            t = timed({"cnet": lambda: net.evaluate(b, m, lg), "mlp": lambda: mlp.evaluate(b, m, lg),
                       "torch_f32": lambda: torch_trip(module, torch.float32, False),
                       "torch_bf16_cl": lambda: torch_trip(half, torch.bfloat16, True)})
            mf = sum(mfma_per_row(N, C, B).values())
            row = {"C": C, "B": B, "rows": R, "cnet_ms": t["cnet"], "mlp_256x2_ms": t["mlp"],
                   "torch_f32_ms": t["torch_f32"], "torch_bf16_channels_last_ms": t["torch_bf16_cl"],
                   "torch_f32_over_cnet": t["torch_f32"]["median"] / t["cnet"]["median"],
                   "torch_bf16_over_cnet": t["torch_bf16_cl"]["median"] / t["cnet"]["median"],
                   "cnet_over_mlp": t["cnet"]["median"] / t["mlp"]["median"],
                   "cnet_tera_ops": 2 * 16384 * mf * R / (t["cnet"]["median"] * 1e-3) / 1e12}
            res["eval"].append(row)
            print(row, flush=True)
            write()
    if not a.skip_search:
        for E in SEARCH_BOARDS:
            for (C, B), (module, half, net) in modules.items():
                env = VecOthelloEnv(E, board_size=N, seed=3, device=dev)
                env.reset()
                env.step_policy("random", 12, record=False)
                float_eval = module.evaluator()
                t = timed({"cnet": lambda: env.puct_search(net, SIMS, layout=None),
                           "torch_f32": lambda: env.puct_search(float_eval, SIMS, layout=None)}, wall=True)
                row = {"boards": E, "C": C, "B": B, "cnet_wall_ms": t["cnet"], "torch_f32_wall_ms": t["torch_f32"],
                       "torch_f32_over_cnet": t["torch_f32"]["median"] / t["cnet"]["median"]}
                res["search"].append(row)
                print(row, flush=True)
                write()
                env.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
