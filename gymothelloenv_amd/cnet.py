"""The int8 residual convolutional policy-value network evaluated on the device
(oth_cnet_blob_bytes / oth_cnet_pack / oth_cnet_eval; include/othello_mi355x.h
defines it in integers).

    DeviceConvNet     the evaluator: int8 weights packed once, rows in the exchange
                      format in, the priors and values of puct_advance out, one launch
    ConvPolicyValue   the float torch module (3 x 3 convs, residual blocks) on
                      net_features' planes that a learner trains
    DeviceConvNet.from_module   the one as the other

A DeviceConvNet is an evaluator of VecOthelloEnv.puct_search / puct_play and of the
batch loop exactly as a DeviceNet is (`quantized = True`, begin with layout=None)."""
import ctypes

import torch

from . import _lib as L
from .net import ACT_MAX, LOGIT_SCALE, _ptr, _q8, _q32, _scale_exp, _stream, net_features

HEAD_OUT = 16  # the head's outputs a square: the logit and 15 value features


class ConvPolicyValue(torch.nn.Module):
    """The float network a learner trains: a 3 x 3 stem conv 3 -> C, `blocks`
    residual blocks of two 3 x 3 convs C -> C, and a 3 x 3 head conv C -> 16, all
    with padding=1.  Every activation is the clipped ReLU clamp(y, 0, 127/128); a
    block is t = clamp(conv(h)), h = clamp(conv(t) + h).  Head output 0 is the
    square's logit (in nats), outputs 1 .. 15, clipped, are the value's features:
    value = clamp(Linear(15 N*N -> 1), -1, 1), the feature of (square a, j) at index
    15 a + j - 1.  forward(x) takes net_features(...) as (R, 3, N, N) (or flat, (R,
    3 N*N)) and returns (logits (R, N*N), values (R,)), the pair puct_quantize
    takes; evaluator() wraps it as an evaluator on leaves.
    DeviceConvNet.from_module(module) makes the integer network of it."""

    def __init__(self, board_size, channels=64, blocks=4):
        super().__init__()
        n = int(board_size)
        self.board_size, self.channels, self.n_blocks = n, int(channels), int(blocks)
        if self.channels not in (64, 128):
            raise ValueError("channels must be 64 or 128")
        if not 1 <= self.n_blocks <= L.OTH_CNET_MAX_BLOCKS:
            raise ValueError("blocks must be in [1, %d]" % L.OTH_CNET_MAX_BLOCKS)
        C = self.channels
        self.stem = torch.nn.Conv2d(3, C, 3, padding=1)
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(C, C, 3, padding=1) for _ in range(2 * self.n_blocks))
        self.head = torch.nn.Conv2d(C, HEAD_OUT, 3, padding=1)
        self.value = torch.nn.Linear(15 * n * n, 1)

    def forward(self, x):
        n = self.board_size
        x = x.reshape(-1, 3, n, n)
        h = torch.clamp(self.stem(x), 0.0, ACT_MAX)
        for k in range(self.n_blocks):
            t = torch.clamp(self.convs[2 * k](h), 0.0, ACT_MAX)
            h = torch.clamp(self.convs[2 * k + 1](t) + h, 0.0, ACT_MAX)
        u = self.head(h)
        R = u.shape[0]
        f = torch.clamp(u[:, 1:], 0.0, ACT_MAX).permute(0, 2, 3, 1).reshape(R, 15 * n * n)
        return u[:, 0].reshape(R, n * n), torch.clamp(self.value(f).squeeze(-1), -1.0, 1.0)

    def evaluator(self):
        """evaluate(leaves) -> (logits, values) for puct_search: the float round trip."""
        def evaluate(leaves):
            p = next(self.parameters())
            x = net_features(leaves.boards, leaves.meta, leaves.legal, self.board_size).to(p.dtype)
            with torch.no_grad():
                return self.forward(x)
        return evaluate


class DeviceConvNet(object):
    """The integer convolutional network on the device.  weights: int8 arrays
    (tensors or numpy) -- the stem (C, 3, 3, 3) as (o, i, ky, kx), 2 B convs (C, C,
    3, 3), the head (16, C, 3, 3), then wv (N*N, 15); biases: int32 arrays (C,), 2 B
    of (C,), (16,), (1,), each |b| <= 2^30; shift_stem, shifts (2 B ints),
    shift_head, policy_shift and value_shift in [0, 24].  The weights are packed
    once, on the host, and kept as a device tensor (`blob`).

    net(leaves) -> (priors int32 (R, N*N), values int32 (R,)) for a PuctLeaves or a
    ReplayBatch (anything with boards, meta and legal): exactly what puct_advance /
    puct_advance_batch take.  One launch, no synchronisation, capturable."""

    quantized = True  # puct_search / puct_play: the outputs are the advance's integers, not logits

    def __init__(self, board_size, weights, biases, shift_stem, shifts, shift_head, policy_shift, value_shift,
                 device=None):
        self._lib = L.load()
        self.board_size = n = int(board_size)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.params, w, b = self.flatten(n, weights, biases, shift_stem, shifts, shift_head, policy_shift, value_shift)
        need = ctypes.c_uint64(0)
        L.check(self._lib.oth_cnet_blob_bytes(n, ctypes.byref(self.params), ctypes.byref(need)), "oth_cnet_blob_bytes")
        host = torch.empty(need.value + 16, dtype=torch.uint8)
        at = (-host.data_ptr()) % 16
        host = host[at:at + need.value]
        L.check(self._lib.oth_cnet_pack(n, ctypes.byref(self.params), _ptr(w), _ptr(b), _ptr(host), need.value),
                "oth_cnet_pack")
        self.blob = host.to(self.device)
        self.channels, self.blocks = self.params.channels, self.params.blocks
        self.shift_stem, self.shifts, self.shift_head = int(shift_stem), [int(s) for s in shifts], int(shift_head)
        self.policy_shift, self.value_shift = int(policy_shift), int(value_shift)

    @staticmethod
    def flatten(board_size, weights, biases, shift_stem, shifts, shift_head, policy_shift, value_shift):
        """The arguments checked and as oth_cnet_pack takes them, without a device:
        (OthCnetParams, w int8 flat, b int32 flat), tensors on the host."""
        n = int(board_size)
        nn = n * n
        ws = [torch.as_tensor(w).detach().cpu() for w in weights]
        bs = [torch.as_tensor(b).detach().cpu() for b in biases]
        shifts = [int(s) for s in shifts]
        blocks = len(shifts) // 2
        C = int(ws[0].shape[0]) if ws and ws[0].dim() == 4 else 0
        if blocks < 1 or len(shifts) != 2 * blocks or len(ws) != 2 * blocks + 3 or len(bs) != 2 * blocks + 3:
            raise ValueError("weights and biases must have 2 B + 3 entries and shifts 2 B, B >= 1")
        shapes = [(C, 3, 3, 3)] + [(C, C, 3, 3)] * (2 * blocks) + [(HEAD_OUT, C, 3, 3), (nn, 15)]
        bshapes = [(C,)] * (2 * blocks + 1) + [(HEAD_OUT,), (1,)]
        for w, b, shape, bshape in zip(ws, bs, shapes, bshapes):
            if tuple(w.shape) != shape or tuple(b.shape) != bshape:
                raise ValueError("expected weights of shape %r and biases of %r" % (shape, bshape))
            if w.dtype.is_floating_point or b.dtype.is_floating_point:
                raise ValueError("weights and biases must be integers (DeviceConvNet.from_module converts a float "
                                 "module)")
            if int(w.min()) < -128 or int(w.max()) > 127:
                raise ValueError("weights must be in [-128, 127]")
            if int(b.abs().max()) > L.OTH_NET_BIAS_MAX:
                raise ValueError("biases must be in [-2^30, 2^30]")
        params = L.OthCnetParams(C, blocks, int(shift_stem), (ctypes.c_int32 * 16)(*(shifts + [0] * (16 - len(shifts)))),
                                 int(shift_head), int(policy_shift), int(value_shift))
        w = torch.cat([x.reshape(-1).to(torch.int8) for x in ws]).contiguous()
        b = torch.cat([x.reshape(-1).to(torch.int32) for x in bs]).contiguous()
        return params, w, b

    def evaluate(self, boards, meta, legal, logits=False):
        """Rows in the exchange format on this device -- boards int64 (R, 2W), meta
        int16 (R,), legal int64 (R, W) -- to (priors int32 (R, N*N), values int32
        (R,)), and with logits=True the int32 (R, N*N + 1) z as a third."""
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
            L.check(self._lib.oth_cnet_eval(n, R, ctypes.byref(self.params), _ptr(self.blob), self.blob.numel(), _ptr(bd),
                                            _ptr(mt), _ptr(lg), _ptr(priors), _ptr(values), _ptr(lo),
                                            _stream(self.device)), "oth_cnet_eval")
        return (priors, values, lo) if logits else (priors, values)

    def __call__(self, leaves):
        return self.evaluate(leaves.boards, leaves.meta, leaves.legal)

    @staticmethod
    def quantize_module(module):
        """from_module's integers without a device: (weights, biases, shift_stem,
        shifts, shift_head, policy_shift, value_shift), tensors on the host."""
        def wb(m):
            return m.weight.detach().double().cpu(), m.bias.detach().double().cpu()

        with torch.no_grad():
            sw, sb = wb(module.stem)
            convs = [wb(c) for c in module.convs]
            hw, hb = wb(module.head)
            vw, vb = wb(module.value)
        s = _scale_exp(sw, 7, 7 + L.OTH_NET_MAX_SHIFT)
        weights, biases, shift_stem, shifts = [_q8(sw, s)], [_q32(sb, s)], s - 7, []
        for w, b in convs:
            s = _scale_exp(w, 0, L.OTH_NET_MAX_SHIFT)
            weights.append(_q8(w, s))
            biases.append(_q32(b, s + 7))
            shifts.append(s)
        tp = _scale_exp(hw[:1] * LOGIT_SCALE, -7, L.OTH_NET_MAX_SHIFT - 7)
        sh = _scale_exp(hw[1:], 0, L.OTH_NET_MAX_SHIFT)
        weights.append(torch.cat([_q8(hw[:1] * LOGIT_SCALE, tp), _q8(hw[1:], sh)]))
        biases.append(torch.cat([_q32(hb[:1] * LOGIT_SCALE, tp + 7), _q32(hb[1:], sh + 7)]))
        tv = _scale_exp(vw, 8, L.OTH_NET_MAX_SHIFT + 8)
        n = module.board_size
        weights.append(_q8(vw, tv).reshape(n * n, 15))
        biases.append(_q32(vb, tv + 7))
        return weights, biases, shift_stem, shifts, sh, tp + 7, tv - 8

    @classmethod
    def from_module(cls, module, device=None):
        """The integer network of a ConvPolicyValue, by DeviceNet.from_module's rule:
        one power-of-two scale a conv (two in the head: its logit row and its 15
        feature rows), an activation a in [0, 127/128] is the integer 128 a, every scale
        exponent is the largest that keeps max|w| 2^s <= 127 within the range its shift
        allows -- beyond it the weights clip:

          stem        w = round(W 2^s), b = round(B 2^s), shift_stem = s - 7, s in [7, 31]
                      (inputs are 0 or 1, so the sum is 2^s y and 128 y = sum >> (s - 7))
          a conv      w = round(W 2^s), b = round(B 2^(s + 7)), shift = s, s in [0, 24]; the
                      second conv of a block the same, so that acc >> shift is in the
                      128-units of the h it is added to
          head row 0  w = round(k W 2^t), b = round(k B 2^(t + 7)), k = 256 log2(e),
                      policy_shift = t + 7, t in [-7, 17] (as DeviceNet's policy rows)
          head 1..15  w = round(W 2^s), b = round(B 2^(s + 7)), shift_head = s, s in [0, 24]
          value       wv = round(W 2^t), bv = round(B 2^(t + 7)), value_shift = t - 8, t in
                      [8, 32]: z >> value_shift is 2^15 v (value weights beyond 127/256 clip)

        Rounding is to nearest, weights clamp to [-128, 127], biases to +-2^30.  A
        module whose weights lie on such a grid converts without loss but for the floor
        of `>> shift`, which is exact where shift = 0."""
        weights, biases, shift_stem, shifts, sh, ps, vs = cls.quantize_module(module)
        return cls(module.board_size, weights, biases, shift_stem, shifts, sh, ps, vs, device=device)
