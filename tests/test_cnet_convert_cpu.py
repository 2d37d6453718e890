"""DeviceConvNet.from_module's rule (gymothelloenv_amd/cnet.py), without a GPU: (a) a
module whose weights lie on the int8 grid with power-of-two scales converts without
loss -- the integer logits are the module's own arithmetic in float64; (b) a
default-initialised module's converted priors and values (through tests/cnet_ref.py)
stay near puct_quantize of the float module.

Run as a program, this file prints (b)'s measurement over the listed seeds as JSON
(the "convert" entry of profiles/cnet.json)."""
import json
import sys

import numpy as np
import pytest
import torch

import cnet_ref as cr
from test_net_convert_cpu import positions, tensors

# (b): the largest |prior - prior'| (units of 1 / 65535) and |value - value'| (units of 2^-15) between the converted
# network and puct_quantize of the float32 module, measured over default-initialised modules of seeds 0 .. 4 on 256
# positions of random play (game seed 0), per (N, channels, blocks) (profiles/cnet.json "convert"):
#   (6, 64, 2): 172, 309    (8, 64, 2): 178, 247    (8, 128, 1): 167, 206
# The bound is twice that, for seeds and positions that are not in the list.
MEASURED = {(6, 64, 2): (172, 309), (8, 64, 2): (178, 247), (8, 128, 1): (167, 206)}
LISTED_SEEDS, LISTED_GAME = (0, 1, 2, 3, 4), 0
OTHER_SEEDS, OTHER_GAME = (5, 6), 1
COUNT = 256


def as_ref(module):
    from gymothelloenv_amd.cnet import DeviceConvNet
    weights, biases, shift_stem, shifts, sh, ps, vs = DeviceConvNet.quantize_module(module)
    return cr.ConvNet(module.board_size, [w.numpy() for w in weights], [b.numpy() for b in biases], shift_stem, shifts,
                      sh, ps, vs)


def deltas(n, channels, blocks, seed, rows):
    """(max |prior difference|, max |value difference|) of one default-initialised module."""
    from gymothelloenv_amd.cnet import ConvPolicyValue
    from gymothelloenv_amd.net import net_features
    from gymothelloenv_amd.vec_env import puct_quantize
    torch.manual_seed(seed)
    module = ConvPolicyValue(n, channels, blocks)
    b, m, lg = tensors(*rows)
    with torch.no_grad():
        logits, values = module(net_features(b, m, lg, n).reshape(-1, 3, n, n))
    want_p, want_v = puct_quantize(logits, lg, values)
    priors, vals, _ = as_ref(module).evaluate(*rows)
    return (int(np.abs(priors.astype(np.int64) - want_p.numpy()).max()),
            int(np.abs(vals.astype(np.int64) - want_v.numpy()).max()))


def measure(seeds, game_seed):
    out = {}
    for n, channels, blocks in sorted(MEASURED):
        rows = positions(n, game_seed, count=COUNT)
        d = [deltas(n, channels, blocks, s, rows) for s in seeds]
        out[(n, channels, blocks)] = (max(x[0] for x in d), max(x[1] for x in d))
    return out


def test_grid_weights_convert_without_loss():
    """The stem at scale 2^-7, the blocks' convs and the head's feature rows in integers (scale 2^0: the only scale
    at which `>> shift` floors nothing), the logit row at 2^-2 / (256 log2 e) and the value at 2^-9: the integer
    logits are the module's float64 logits times their scale."""
    from gymothelloenv_amd.cnet import ConvPolicyValue, DeviceConvNet
    from gymothelloenv_amd.net import ACT_MAX, LOGIT_SCALE, net_features
    n, C, B = 6, 64, 2
    nn = n * n
    gen = np.random.default_rng(7)
    module = ConvPolicyValue(n, C, B).double()

    def grid(shape, lo, hi, keep=1.0):  # (-128 would halve the scale that keeps max|w| 2^s <= 127)
        q = gen.integers(lo, hi, size=shape) * (gen.random(shape) < keep)
        q.flat[0] = 127
        return q

    def put(conv, q, scale, k, bias_scale):
        conv.weight.copy_(torch.from_numpy(q.astype(np.float64) * scale))
        conv.bias.copy_(torch.from_numpy(k * bias_scale))

    with torch.no_grad():
        qs, ks = grid((C, 3, 3, 3), -16, 17), gen.integers(-40, 41, size=C)
        put(module.stem, qs, 2.0 ** -7, ks, 1 / 128.0)
        convs = []
        for conv in module.convs:  # sparse, so that the sums of shift 0 do not all leave [0, 127]
            q, k = grid((C, C, 3, 3), -1, 2, keep=0.02), gen.integers(-30, 31, size=C)
            put(conv, q, 1.0, k, 1 / 128.0)
            convs.append((q, k))
        qh, kh = grid((16, C, 3, 3), -1, 2, keep=0.05), gen.integers(-2 ** 10, 2 ** 10, size=16)
        qh[0] = gen.integers(-127, 128, size=(C, 3, 3))
        qh[0].flat[0] = 127
        qh[1].flat[0] = 127
        scale_h = np.array([2.0 ** -2 / LOGIT_SCALE] + [1.0] * 15)
        module.head.weight.copy_(torch.from_numpy(qh * scale_h[:, None, None, None]))
        module.head.bias.copy_(torch.from_numpy(kh * np.array([2.0 ** -9 / LOGIT_SCALE] + [1 / 128.0] * 15)))
        qv, kv = grid((1, 15 * nn), -127, 128), gen.integers(-2 ** 14, 2 ** 14, size=1)
        module.value.weight.copy_(torch.from_numpy(qv * 2.0 ** -9))
        module.value.bias.copy_(torch.from_numpy(kv / 2.0 ** 16))
    weights, biases, shift_stem, shifts, sh, ps, vs = DeviceConvNet.quantize_module(module)
    assert (shift_stem, shifts, sh, ps, vs) == (0, [0] * (2 * B), 0, 9, 1)
    np.testing.assert_array_equal(weights[0].numpy(), qs)
    np.testing.assert_array_equal(biases[0].numpy(), ks)
    for (q, k), w, b in zip(convs, weights[1:], biases[1:]):
        np.testing.assert_array_equal(w.numpy(), q)
        np.testing.assert_array_equal(b.numpy(), k)
    np.testing.assert_array_equal(weights[-2].numpy(), qh)
    np.testing.assert_array_equal(biases[-2].numpy(), kh)
    np.testing.assert_array_equal(weights[-1].numpy(), qv.reshape(nn, 15))
    np.testing.assert_array_equal(biases[-1].numpy(), kv)
    rows = positions(n, 3, count=128)
    ref = as_ref(module)
    z = ref.logits(*rows)
    with torch.no_grad():
        x = net_features(*tensors(*rows), n).double().reshape(-1, 3, n, n)
        h = torch.clamp(module.stem(x), 0.0, ACT_MAX)
        for k in range(B):
            t = torch.clamp(module.convs[2 * k](h), 0.0, ACT_MAX)
            h = torch.clamp(module.convs[2 * k + 1](t) + h, 0.0, ACT_MAX)
        u = module.head(h)
        f = torch.clamp(u[:, 1:], 0.0, ACT_MAX).permute(0, 2, 3, 1).reshape(-1, 15 * nn)
        lp = (u[:, 0].reshape(-1, nn) * (LOGIT_SCALE * 2.0 ** 9)).numpy()
        lv = (module.value(f) * 2.0 ** 16).numpy()
        logits, values = module(x)
        np.testing.assert_array_equal(logits.numpy(), u[:, 0].reshape(-1, nn).numpy())  # forward is this graph
    assert np.abs(lp - z[:, :nn]).max() < 1e-4 and np.abs(lv[:, 0] - z[:, nn]).max() < 1e-9
    acts = [act for _, _, act in ref.layers(*rows)[0]]
    assert all(((a > 0) & (a < 127)).mean() > 0.05 for a in acts)  # (the activations are not all clipped)
    assert len(set(z[:, 0].tolist())) > 16


@pytest.mark.parametrize("n,channels,blocks", sorted(MEASURED))
def test_default_modules_stay_near_the_float_module(n, channels, blocks):
    rows = positions(n, OTHER_GAME, count=COUNT)
    got = [deltas(n, channels, blocks, s, rows) for s in OTHER_SEEDS]
    dp, dv = max(x[0] for x in got), max(x[1] for x in got)
    print("N = %d C = %d B = %d: max |prior difference| %d, max |value difference| %d" % (n, channels, blocks, dp, dv))
    assert dp <= 2 * MEASURED[(n, channels, blocks)][0] and dv <= 2 * MEASURED[(n, channels, blocks)][1]


def test_python_surface():
    import inspect

    import gymothelloenv_amd as g
    from gymothelloenv_amd import cnet
    assert g.DeviceConvNet is cnet.DeviceConvNet and g.ConvPolicyValue is cnet.ConvPolicyValue
    assert cnet.DeviceConvNet.quantized is True
    names = list(inspect.signature(cnet.DeviceConvNet.__init__).parameters)[1:]
    assert names == ["board_size", "weights", "biases", "shift_stem", "shifts", "shift_head", "policy_shift",
                     "value_shift", "device"]
    assert list(inspect.signature(cnet.DeviceConvNet.evaluate).parameters)[1:] == ["boards", "meta", "legal", "logits"]
    assert list(inspect.signature(cnet.ConvPolicyValue.__init__).parameters)[1:] == ["board_size", "channels", "blocks"]
    with pytest.raises(ValueError):
        cnet.ConvPolicyValue(8, 96, 2)
    with pytest.raises(ValueError):
        cnet.ConvPolicyValue(8, 64, 9)


if __name__ == "__main__":
    m = measure(LISTED_SEEDS, LISTED_GAME)
    json.dump({"seeds": list(LISTED_SEEDS), "game_seed": LISTED_GAME, "positions": COUNT,
               "max_abs_prior_difference_of_65535": {"N%d_C%d_B%d" % k: v[0] for k, v in sorted(m.items())},
               "max_abs_value_difference_of_32768": {"N%d_C%d_B%d" % k: v[1] for k, v in sorted(m.items())}},
              sys.stdout, indent=1)
    print()
