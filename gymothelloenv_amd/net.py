"""The int8 policy-value network evaluated on the device (oth_net_blob_bytes /
oth_net_pack / oth_net_eval; include/othello_mi355x.h defines it in integers).

    DeviceNet        the evaluator: int8 weights packed once, rows in the exchange
                     format in, the priors and values of puct_advance out, one launch
    net_features     the network's 3 N*N inputs as a float tensor, for training
    MLPPolicyValue   the float torch module on those features that a learner trains
    DeviceNet.from_module   the one as the other
    NetPlayer        a DeviceNet (or a cnet.DeviceConvNet) as a player:
                     VecOthelloEnv.play_net, and the embedded opponent of reset_vs /
                     step_vs (oth_play_net, oth_reset_vs_net, oth_step_vs_net; for a
                     conv net oth_play_cnet, oth_reset_vs_cnet, oth_step_vs_cnet)

A DeviceNet is an evaluator of VecOthelloEnv.puct_search / puct_play whose outputs
go to the advance as they are (`quantized = True`): no float lies between the
boards and the visit counts, and it needs no observation (begin with layout=None)."""
import ctypes
import math

import torch

from . import _lib as L

ACT_MAX = 127.0 / 128.0  # the clipped ReLU's upper end: the largest int8 activation (128 stands for 1.0)
LOGIT_SCALE = 256.0 * math.log2(math.e)  # integer-softmax units (1/256 octave) per nat


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def net_features(boards, meta, legal, board_size):
    """The network's inputs in torch: float32 (R, 3 N*N) of 0 and 1 -- the mover's
    discs, the opponent's, the legal squares (the mover's words are the white words
    where meta bit 0 is set) -- from rows in the exchange format: boards int64 (R,
    2W), meta int16 (R,), legal int64 (R, W), as PuctLeaves and ReplayBatch carry
    them.  Bits off the board are not read."""
    n = int(board_size)
    nn, W = n * n, (n * n + 63) // 64
    R = meta.numel()
    b = boards.reshape(R, 2 * W)
    white = (meta.reshape(R, 1).to(torch.int64) & 1).bool()
    mover = torch.where(white, b[:, W:], b[:, :W])
    opp = torch.where(white, b[:, :W], b[:, W:])
    a = torch.arange(nn, device=b.device)
    planes = [(w[:, a // 64] >> (a % 64)) & 1 for w in (mover, opp, legal.reshape(R, W))]
    return torch.cat(planes, dim=1).to(torch.float32)


class MLPPolicyValue(torch.nn.Module):
    """The float network a learner trains: `layers` hidden Linear layers of width
    `hidden` on net_features' 3 N*N inputs, each followed by the clipped ReLU
    clamp(y, 0, 127/128), a policy head (N*N logits, in nats) and a value head
    clamped to [-1, 1].  forward(features) -> (logits (R, N*N), values (R,)), the pair
    puct_quantize takes; evaluator() wraps it as an evaluator on leaves.
    DeviceNet.from_module(module) makes the integer network of it."""

    def __init__(self, board_size, hidden=256, layers=2):
        super().__init__()
        n = int(board_size)
        self.board_size, self.width, self.n_layers = n, int(hidden), int(layers)
        if not 1 <= self.n_layers <= L.OTH_NET_MAX_LAYERS:
            raise ValueError("layers must be in [1, %d]" % L.OTH_NET_MAX_LAYERS)
        if self.width % 64 or not 64 <= self.width <= L.OTH_NET_MAX_WIDTH:
            raise ValueError("hidden must be a multiple of 64 in [64, %d]" % L.OTH_NET_MAX_WIDTH)
        sizes = [3 * n * n] + [self.width] * self.n_layers
        self.hidden = torch.nn.ModuleList(torch.nn.Linear(i, o) for i, o in zip(sizes[:-1], sizes[1:]))
        self.policy = torch.nn.Linear(self.width, n * n)
        self.value = torch.nn.Linear(self.width, 1)

    def forward(self, features):
        x = features
        for lin in self.hidden:
            x = torch.clamp(lin(x), 0.0, ACT_MAX)
        return self.policy(x), torch.clamp(self.value(x).squeeze(-1), -1.0, 1.0)

    def evaluator(self):
        """evaluate(leaves) -> (logits, values) for puct_search: the float round trip."""
        def evaluate(leaves):
            p = next(self.parameters())
            x = net_features(leaves.boards, leaves.meta, leaves.legal, self.board_size).to(p.dtype)
            with torch.no_grad():
                return self.forward(x)
        return evaluate


def _scale_exp(w, lo, hi):
    """The largest s in [lo, hi] with max|w| 2^s <= 127 (lo where there is none: the weights clip)."""
    m = float(w.abs().max())
    if m == 0.0:
        return hi
    return max(lo, min(hi, int(math.floor(math.log2(127.0 / m) + 1e-9))))  # (a grid weight of 127 stays 127)


def _q8(w, s):
    return torch.clamp(torch.round(w * 2.0 ** s), -128, 127).to(torch.int8)


def _q32(b, s):
    return torch.clamp(torch.round(b * 2.0 ** s), -L.OTH_NET_BIAS_MAX, L.OTH_NET_BIAS_MAX).to(torch.int32)


class DeviceNet(object):
    """The integer network on the device.  weights: L + 1 int8 arrays (tensors or
    numpy) w[0] (H, 3 N*N), w[l] (H, H), then the head (N*N + 1, H); biases: L + 1
    int32 arrays (H,) .. (N*N + 1,), each |b| <= 2^30; shifts: L ints in [0, 24];
    policy_shift and value_shift in [0, 24].  The weights are packed once, on the
    host, and kept as a device tensor (`blob`).

    net(leaves) -> (priors int32 (R, N*N), values int32 (R,)) for a PuctLeaves or a
    ReplayBatch (anything with boards, meta and legal): exactly what puct_advance /
    puct_advance_batch take.  One launch, no synchronisation, capturable."""

    quantized = True  # puct_search / puct_play: the outputs are the advance's integers, not logits

    def __init__(self, board_size, weights, biases, shifts, policy_shift, value_shift, device=None):
        self._lib = L.load()
        self.board_size = n = int(board_size)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        ws = [torch.as_tensor(w).detach().cpu() for w in weights]
        bs = [torch.as_tensor(b).detach().cpu() for b in biases]
        nn = n * n
        layers, width = len(ws) - 1, int(ws[0].shape[0]) if ws and ws[0].dim() == 2 else 0
        shifts = [int(s) for s in shifts]
        if layers < 1 or len(bs) != layers + 1 or len(shifts) != layers:
            raise ValueError("weights and biases must have L + 1 entries and shifts L, L >= 1")
        shapes = [(width, 3 * nn)] + [(width, width)] * (layers - 1) + [(nn + 1, width)]
        for w, b, shape in zip(ws, bs, shapes):
            if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
                raise ValueError("expected weights of shape %r and biases of %r" % (shape, shape[:1]))
            if w.dtype.is_floating_point or b.dtype.is_floating_point:
                raise ValueError("weights and biases must be integers (DeviceNet.from_module converts a float module)")
            if int(w.min()) < -128 or int(w.max()) > 127:
                raise ValueError("weights must be in [-128, 127]")
            if int(b.abs().max()) > L.OTH_NET_BIAS_MAX:
                raise ValueError("biases must be in [-2^30, 2^30]")
        self.params = L.OthNetParams(layers, width, (ctypes.c_int32 * 4)(*(shifts + [0] * (4 - layers))),
                                     int(policy_shift), int(value_shift))
        need = ctypes.c_uint64(0)
        L.check(self._lib.oth_net_blob_bytes(n, ctypes.byref(self.params), ctypes.byref(need)), "oth_net_blob_bytes")
        w = torch.cat([x.reshape(-1).to(torch.int8) for x in ws]).contiguous()
        b = torch.cat([x.reshape(-1).to(torch.int32) for x in bs]).contiguous()
        host = torch.empty(need.value + 16, dtype=torch.uint8)
        at = (-host.data_ptr()) % 16
        host = host[at:at + need.value]
        L.check(self._lib.oth_net_pack(n, ctypes.byref(self.params), _ptr(w), _ptr(b), _ptr(host), need.value),
                "oth_net_pack")
        self.blob = host.to(self.device)
        self.layers, self.width, self.shifts = layers, width, shifts
        self.policy_shift, self.value_shift = int(policy_shift), int(value_shift)

    def evaluate(self, boards, meta, legal, logits=False):
        """Rows in the exchange format on this device -- boards int64 (R, 2W), meta
        int16 (R,), legal int64 (R, W) -- to (priors int32 (R, N*N), values int32
        (R,)), and with logits=True the head's int32 (R, N*N + 1) as a third."""
        n = self.board_size
        nn, W = n * n, (n * n + 63) // 64
        R = int(meta.numel())
        bd = boards.to(device=self.device, dtype=torch.int64).contiguous()
        mt = meta.to(device=self.device, dtype=torch.int16).contiguous()
        lg = legal.to(device=self.device, dtype=torch.int64).contiguous()
        if bd.numel() != R * 2 * W or lg.numel() != R * W:
            raise ValueError("boards must have %d elements and legal %d" % (R * 2 * W, R * W))
        priors = torch.empty(R, nn, dtype=torch.int32, device=self.device)
        values = torch.empty(R, dtype=torch.int32, device=self.device)
        lo = torch.empty(R, nn + 1, dtype=torch.int32, device=self.device) if logits else None
        with torch.cuda.device(self.device):
            L.check(self._lib.oth_net_eval(n, R, ctypes.byref(self.params), _ptr(self.blob), self.blob.numel(), _ptr(bd),
                                           _ptr(mt), _ptr(lg), _ptr(priors), _ptr(values), _ptr(lo),
                                           _stream(self.device)), "oth_net_eval")
        return (priors, values, lo) if logits else (priors, values)

    def __call__(self, leaves):
        return self.evaluate(leaves.boards, leaves.meta, leaves.legal)

    @staticmethod
    def quantize_module(module):
        """from_module's integers without a device: (weights, biases, shifts,
        policy_shift, value_shift), tensors on the host."""
        with torch.no_grad():
            hid = [(lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu()) for lin in module.hidden]
            pw, pb = module.policy.weight.detach().double().cpu(), module.policy.bias.detach().double().cpu()
            vw, vb = module.value.weight.detach().double().cpu(), module.value.bias.detach().double().cpu()
        weights, biases, shifts = [], [], []
        for l, (w, b) in enumerate(hid):
            if l == 0:
                s = _scale_exp(w, 7, 7 + L.OTH_NET_MAX_SHIFT)
                weights.append(_q8(w, s))
                biases.append(_q32(b, s))
                shifts.append(s - 7)
            else:
                s = _scale_exp(w, 0, L.OTH_NET_MAX_SHIFT)
                weights.append(_q8(w, s))
                biases.append(_q32(b, s + 7))
                shifts.append(s)
        tp = _scale_exp(pw * LOGIT_SCALE, -7, L.OTH_NET_MAX_SHIFT - 7)
        tv = _scale_exp(vw, 8, L.OTH_NET_MAX_SHIFT + 8)
        weights.append(torch.cat([_q8(pw * LOGIT_SCALE, tp), _q8(vw, tv)]))
        biases.append(torch.cat([_q32(pb * LOGIT_SCALE, tp + 7), _q32(vb, tv + 7)]))
        return weights, biases, shifts, tp + 7, tv - 8

    @classmethod
    def from_module(cls, module, device=None):
        """The integer network of an MLPPolicyValue.  The rule, per layer, with one
        power-of-two scale a layer (an activation a in [0, 127/128] is the integer
        128 a; every scale exponent is the largest that keeps max|w| 2^s <= 127,
        within the range its shift allows -- beyond it the weights clip):

          layer 0      w = round(W 2^s), b = round(B 2^s), shift = s - 7, s in [7, 31]
                       (inputs are 0 or 1, so the sum is 2^s y and 128 y = sum >> (s - 7))
          layer l > 0  w = round(W 2^s), b = round(B 2^(s + 7)), shift = s, s in [0, 24]
          policy rows  w = round(k W 2^t), b = round(k B 2^(t + 7)), k = 256 log2(e):
                       the logits in units of 2^-(t + 7) / 256 octaves, policy_shift = t + 7,
                       t in [-7, 17], so that (m - z) >> policy_shift is 256 log2(e) (l_max - l)
                       and EXP2 gives e^-(l_max - l)
          value row    w = round(W 2^t), b = round(B 2^(t + 7)), value_shift = t - 8, t in [8,
                       32]: z >> value_shift is 2^15 v (value weights beyond 127/256 clip)

        Rounding is to nearest, weights clamp to [-128, 127], biases to +-2^30.  A
        module whose weights lie on such a grid converts without loss but for the floor
        of `>> shift`, which is exact where shift = 0."""
        weights, biases, shifts, ps, vs = cls.quantize_module(module)
        return cls(module.board_size, weights, biases, shifts, ps, vs, device=device)


class NetPlayer(object):
    """A network as a player (struct oth_net_policy, or struct oth_cnet_policy for
    a conv net): the move of a board is the legal square of the largest logit of
    `net` (a DeviceNet or a DeviceConvNet; `kind` is "mlp" or "conv"), the lowest square of
    equals, once the board holds at least `sample_discs` discs; with fewer discs it
    is drawn in proportion to the network's priors (Philox purpose 7, keyed by the
    env's seed, its global id and the ply's index: reproducible and shardable).
    sample_discs = 0 (the default) never samples, 257 always does; on 8 x 8,
    sample_discs = 12 samples the first eight discs placed.  Used by
    VecOthelloEnv.play_net and as `opponent` of reset_vs / step_vs.  The struct is
    built once and keeps the net's packed weights alive, so a captured call copies
    nothing."""

    def __init__(self, net, sample_discs=0):
        from .cnet import DeviceConvNet
        if not isinstance(net, (DeviceNet, DeviceConvNet)):
            raise TypeError("NetPlayer takes a DeviceNet or a DeviceConvNet")
        if isinstance(sample_discs, bool) or int(sample_discs) != sample_discs:
            raise ValueError("sample_discs must be an integer")
        if not 0 <= int(sample_discs) <= L.OTH_NET_SAMPLE_DISCS_MAX:
            raise ValueError("sample_discs must be in [0, %d]" % L.OTH_NET_SAMPLE_DISCS_MAX)
        self.net, self.sample_discs = net, int(sample_discs)
        self.kind = "conv" if isinstance(net, DeviceConvNet) else "mlp"
        struct = L.OthCnetPolicy if self.kind == "conv" else L.OthNetPolicy
        self._struct = struct(net.params, net.blob.data_ptr(), net.blob.numel(), self.sample_discs)

    def _policy(self, env):
        """The struct, for an env of the net's board size on the net's device."""
        if env.board_size != self.net.board_size:
            raise ValueError("the network is for %d x %d boards, the env has %d x %d" % (
                self.net.board_size, self.net.board_size, env.board_size, env.board_size))
        if torch.device(env.device) != self.net.device:
            raise ValueError("the network lives on %s, the env on %s" % (self.net.device, env.device))
        return self._struct

    def __repr__(self):
        if self.kind == "conv":
            return "NetPlayer(<%d x %d, conv, %d blocks of %d channels>, sample_discs=%d)" % (
                self.net.board_size, self.net.board_size, self.net.blocks, self.net.channels, self.sample_discs)
        return "NetPlayer(<%d x %d, %d layers of %d>, sample_discs=%d)" % (
            self.net.board_size, self.net.board_size, self.net.layers, self.net.width, self.sample_discs)
