"""DeviceNet.from_module's rule (gymothelloenv_amd/net.py), without a GPU: (a) a
module whose weights lie on the int8 grid with power-of-two scales converts
without loss -- the integer logits are the module's own arithmetic in float64;
(b) a default-initialised module's converted priors and values (through
tests/net_ref.py) stay near puct_quantize of the float module.

Run as a program, this file prints (b)'s measurement over the listed seeds as JSON
(the "convert" entry of profiles/net.json)."""
import json
import sys

import numpy as np
import pytest
import torch

import net_ref as nr
import replay_cases as rc

# (b): the largest |prior - prior'| (units of 1 / 65535) and |value - value'| (units of 2^-15) between the converted
# network and puct_quantize of the float32 module, measured over default-initialised modules of seeds 0 .. 4 on 512
# positions of random play (game seed 0), per (N, hidden) with two hidden layers (profiles/net.json "convert"):
#   (6, 64): 157, 197    (6, 256): 164, 239    (8, 64): 116, 228    (8, 256): 174, 239
# The bound is twice that, for seeds and positions that are not in the list.
MEASURED = {(6, 64): (157, 197), (6, 256): (164, 239), (8, 64): (116, 228), (8, 256): (174, 239)}
LISTED_SEEDS, LISTED_GAME = (0, 1, 2, 3, 4), 0
OTHER_SEEDS, OTHER_GAME = (5, 6), 1


def positions(n, game_seed, count=512, E=64):
    """`count` positions of random play: E boards with auto-reset, a snapshot every fourth ply."""
    game, gen = rc.OracleGame(n, E, 4, game_seed), np.random.default_rng(100 + game_seed)
    boards, meta, legal = [], [], []
    ply = 0
    while len(boards) * E < count:
        s = game.state()
        if ply % 4 == 3:
            boards.append(s.boards.copy())
            meta.append(s.meta.copy())
            legal.append(s.legal.copy())
        game.step(rc.random_legal(s, gen))
        ply += 1
    return np.concatenate(boards)[:count], np.concatenate(meta)[:count], np.concatenate(legal)[:count]


def as_ref(module):
    from gymothelloenv_amd.net import DeviceNet
    weights, biases, shifts, ps, vs = DeviceNet.quantize_module(module)
    return nr.Net(module.board_size, [w.numpy() for w in weights], [b.numpy() for b in biases], shifts, ps, vs)


def tensors(boards, meta, legal):
    return (torch.from_numpy(boards.view(np.int64)), torch.from_numpy(meta.view(np.int16)),
            torch.from_numpy(legal.view(np.int64)))


def deltas(n, hidden, seed, rows):
    """(max |prior difference|, max |value difference|) of one default-initialised module."""
    from gymothelloenv_amd.net import MLPPolicyValue, net_features
    from gymothelloenv_amd.vec_env import puct_quantize
    torch.manual_seed(seed)
    module = MLPPolicyValue(n, hidden, 2)
    b, m, lg = tensors(*rows)
    with torch.no_grad():
        logits, values = module(net_features(b, m, lg, n))
    want_p, want_v = puct_quantize(logits, lg, values)
    priors, vals, _ = as_ref(module).evaluate(*rows)
    return (int(np.abs(priors.astype(np.int64) - want_p.numpy()).max()),
            int(np.abs(vals.astype(np.int64) - want_v.numpy()).max()))


def measure(seeds, game_seed):
    out = {}
    for n in (6, 8):
        rows = positions(n, game_seed)
        for hidden in (64, 256):
            d = [deltas(n, hidden, s, rows) for s in seeds]
            out[(n, hidden)] = (max(x[0] for x in d), max(x[1] for x in d))
    return out


def test_features_are_the_references():
    from gymothelloenv_amd.net import net_features
    gen = np.random.default_rng(2)
    for n in (4, 6, 8, 9, 16):
        W = nr.nwords(n)
        boards = gen.integers(0, 2 ** 64, size=(19, 2 * W), dtype=np.uint64)
        legal = gen.integers(0, 2 ** 64, size=(19, W), dtype=np.uint64)
        meta = gen.integers(0, 2 ** 16, size=19, dtype=np.uint16)
        got = net_features(*tensors(boards, meta, legal), n)
        assert got.dtype == torch.float32
        np.testing.assert_array_equal(got.numpy(), nr.features(n, boards, meta, legal))


@pytest.mark.parametrize("layers", (1, 2))
def test_grid_weights_convert_without_loss(layers):
    """Layer 0 at scale 2^-7, a second layer of integers (scale 2^0: the only scale at which `>> shift` floors
    nothing), policy rows at 2^-2 / (256 log2 e) and the value row at 2^-9: the integer logits are the module's
    float64 logits times their scale."""
    from gymothelloenv_amd.net import ACT_MAX, LOGIT_SCALE, DeviceNet, MLPPolicyValue, net_features
    n, H = 6, 64
    nn = n * n
    gen = np.random.default_rng(7)
    module = MLPPolicyValue(n, H, layers).double()

    def grid(shape, scale, lo=-127, hi=128):  # (-128 would halve the scale that keeps max|w| 2^s <= 127)
        q = gen.integers(lo, hi, size=shape)
        q.flat[0] = 127
        return q, torch.from_numpy(q.astype(np.float64) * scale)

    ints = []
    with torch.no_grad():
        for l, lin in enumerate(module.hidden):
            scale = 2.0 ** -7 if l == 0 else 1.0
            # (small but for one 127, so that the activations spread)
            q, w = grid(tuple(lin.weight.shape), scale, *((-16, 17) if l == 0 else (-1, 2)))
            k = gen.integers(-60, 61, size=lin.bias.shape)
            lin.weight.copy_(w)
            lin.bias.copy_(torch.from_numpy(k / 128.0))
            ints.append((q, k))
        qp, wp = grid((nn, H), 2.0 ** -2 / LOGIT_SCALE)
        kp = gen.integers(-2 ** 20, 2 ** 20, size=nn)
        module.policy.weight.copy_(wp)
        module.policy.bias.copy_(torch.from_numpy(kp / (2.0 ** 9 * LOGIT_SCALE)))
        qv, wv = grid((1, H), 2.0 ** -9)
        kv = gen.integers(-2 ** 14, 2 ** 14, size=1)
        module.value.weight.copy_(wv)
        module.value.bias.copy_(torch.from_numpy(kv / 2.0 ** 16))
    weights, biases, shifts, ps, vs = DeviceNet.quantize_module(module)
    assert shifts == [0] * layers and ps == 9 and vs == 1
    if layers == 2:  # (the second layer's largest weight is 127 only by grid(): its scale is 2^0)
        assert int(weights[1].abs().max()) == 127
    for (q, k), w, b in zip(ints, weights, biases):
        np.testing.assert_array_equal(w.numpy(), q)
        np.testing.assert_array_equal(b.numpy(), k)
    np.testing.assert_array_equal(weights[-1].numpy(), np.concatenate([qp, qv]))
    np.testing.assert_array_equal(biases[-1].numpy(), np.concatenate([kp, kv]))
    rows = positions(n, 3, count=128)
    ref = as_ref(module)
    z = ref.logits(*rows)
    with torch.no_grad():
        a = net_features(*tensors(*rows), n).double()
        for lin in module.hidden:
            a = torch.clamp(lin(a), 0.0, ACT_MAX)
        lp = (module.policy(a) * (LOGIT_SCALE * 2.0 ** 9)).numpy()
        lv = (module.value(a) * 2.0 ** 16).numpy()
    assert np.abs(lp - z[:, :nn]).max() < 1e-5 and np.abs(lv[:, 0] - z[:, nn]).max() < 1e-9
    assert len(set(z[:, 0].tolist())) > 16  # (the activations are not all clipped)


@pytest.mark.parametrize("n,hidden", sorted(MEASURED))
def test_default_modules_stay_near_the_float_module(n, hidden):
    got = [deltas(n, hidden, s, positions(n, OTHER_GAME)) for s in OTHER_SEEDS]
    dp, dv = max(x[0] for x in got), max(x[1] for x in got)
    print("N = %d hidden = %d: max |prior difference| %d, max |value difference| %d" % (n, hidden, dp, dv))
    assert dp <= 2 * MEASURED[(n, hidden)][0] and dv <= 2 * MEASURED[(n, hidden)][1]


if __name__ == "__main__":
    m = measure(LISTED_SEEDS, LISTED_GAME)
    json.dump({"seeds": list(LISTED_SEEDS), "game_seed": LISTED_GAME, "positions": 512, "layers": 2,
               "max_abs_prior_difference_of_65535": {"N%d_H%d" % k: v[0] for k, v in sorted(m.items())},
               "max_abs_value_difference_of_32768": {"N%d_H%d" % k: v[1] for k, v in sorted(m.items())}},
              sys.stdout, indent=1)
    print()
