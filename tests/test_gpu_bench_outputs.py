"""bench.py's plain run and --dump-outputs on the GPU, in this process: the
line a plain run prints (the headline only), and the dumped arrays against the
same launches made directly on a VecOthelloEnv (seed 0, the bench's inputs)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

E, P, STEPS, WARMUP = 4099, 7, 2, 1  # an odd board count: more than one block, a partial last wave
NAMES = ("actions", "rewards", "dones", "board", "possible_moves", "wdl", "env_ids")


def _bench(capsys, out_dir, extra=()):
    rc = bench.main(["--gpus", "1", "--envs", str(E), "--plies-per-step", str(P), "--steps", str(STEPS),
                     "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)] + list(extra))
    assert rc == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {k: np.load(os.path.join(str(out_dir), k + ".npy")) for k in NAMES}


@pytest.fixture(scope="module")
def direct():
    """The bench's launches made by hand: (last step's outputs, final boards, W/D/L of the timed steps)."""
    import torch
    from gymothelloenv_amd import VecOthelloEnv
    env = VecOthelloEnv(E, board_size=8, auto_reset=True, seed=0, device="cuda:0")
    env.reset()
    for _ in range(WARMUP):
        env.step_policy("random", n_plies=P)
    env.counts(reset=True)
    for _ in range(STEPS):
        a, r, d = env.step_policy("random", n_plies=P)
    ref = {"actions": a, "rewards": r, "dones": d, "board": env.observe("absolute", torch.int64),
           "possible_moves": env.observe("legal", torch.int64), "wdl": env.counts()}
    ref = {k: v.cpu().numpy().astype(np.float64) for k, v in ref.items()}
    env.close()
    return ref


def test_plain_run_line_and_dump_equal_direct_launches(capsys, tmp_path, direct):
    line, got = _bench(capsys, tmp_path)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - E * P) < 1e-6 * E * P  # ms_per_step is one timed step
    for k in ("cpu_baseline", "step_external", "configs", "sustained", "side_summary"):
        assert k not in line, k  # those belong to --full
    assert sorted(os.listdir(str(tmp_path))) == sorted(k + ".npy" for k in NAMES)
    assert np.array_equal(got["env_ids"], np.arange(E))
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        if k != "env_ids":
            assert v.shape == direct[k].shape and np.array_equal(v, direct[k]), k
    assert got["actions"].shape == (P, E) and got["board"].shape == (E, 8, 8)


def test_dump_sample_is_fixed_and_within_budget(capsys, tmp_path, direct, monkeypatch):
    """Beyond the size budget a seeded sample of the boards is written: the
    same boards on every run, each column equal to the full outputs'."""
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    _, one = _bench(capsys, tmp_path / "a")
    _, two = _bench(capsys, tmp_path / "b")
    ids = one["env_ids"].astype(np.int64)
    assert 0 < len(ids) < E and np.all(np.diff(ids) > 0) and ids[-1] < E
    assert sum(v.nbytes for v in one.values()) <= 200_000 + one["wdl"].nbytes
    for k in NAMES:
        assert np.array_equal(one[k], two[k]), k
    for k in ("actions", "rewards", "dones"):
        assert np.array_equal(one[k], direct[k][:, ids]), k
    for k in ("board", "possible_moves"):
        assert np.array_equal(one[k], direct[k][ids]), k
    assert np.array_equal(one["wdl"], direct["wdl"])
