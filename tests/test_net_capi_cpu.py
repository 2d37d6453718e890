"""The network's C ABI without a GPU: oth_net_blob_bytes and oth_net_pack, which
run on the host, every argument check of oth_net_eval (with nothing launched), and
the Python surface."""
import ctypes
import inspect
import threading

import numpy as np
import pytest

import net_cases as nc
from test_net_host import load_hostlib, params as host_params, ptr


@pytest.fixture(scope="module")
def lib():
    from gymothelloenv_amd import _lib
    from gymothelloenv_amd import build as hb
    if hb.needs_build():
        hb.build()
    return _lib.load(require_gpu=False)


def on_a_thread(fn):
    """oth_last_error is per thread: rejected calls run on a thread of their own."""
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    assert len(out) == 1
    return out[0]


def params(L=2, H=128, shifts=(5, 9), policy_shift=8, value_shift=3):
    from gymothelloenv_amd import _lib as L_
    sh = list(shifts) + [0] * (4 - len(shifts))
    return L_.OthNetParams(L, H, (ctypes.c_int32 * 4)(*sh), policy_shift, value_shift)


BAD_PARAMS = [("layers = 0", dict(L=0), b"layers"), ("layers = 5", dict(L=5, shifts=(0,) * 4), b"layers"),
              ("width = 32", dict(H=32), b"width"), ("width = 96", dict(H=96), b"width"),
              ("width = 576", dict(H=576), b"width"), ("shift = 25", dict(shifts=(5, 25)), b"shift"),
              ("shift = -1", dict(shifts=(-1, 9)), b"shift"), ("policy_shift = 25", dict(policy_shift=25), b"policy_shift"),
              ("policy_shift = -1", dict(policy_shift=-1), b"policy_shift"),
              ("value_shift = 25", dict(value_shift=25), b"value_shift"),
              ("value_shift = -1", dict(value_shift=-1), b"value_shift")]


def test_blob_bytes(lib):
    from gymothelloenv_amd import _lib as L
    assert (L.OTH_NET_MAX_LAYERS, L.OTH_NET_MAX_WIDTH, L.OTH_NET_MAX_SHIFT) == (4, 512, 24)
    assert (L.OTH_NET_BIAS_MAX, L.OTH_NET_MAX_ROWS) == (1 << 30, 1 << 24)
    S = L.OthNetParams
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("layers", 0), ("width", 4), ("shift", 8),
                                                                   ("policy_shift", 24), ("value_shift", 28)]

    def size(n, p):
        b = ctypes.c_uint64(0)
        return lib.oth_net_blob_bytes(n, None if p is None else ctypes.byref(p), ctypes.byref(b)), b.value

    for n in range(4, 17):
        for Ln in range(1, 5):
            for H in (64, 192, 512):
                assert size(n, params(Ln, H, (3,) * Ln)) == (0, nc.blob_bytes(n, Ln, H)), (n, Ln, H)
    assert size(8, params(2, 128, (24, 0, 99, -5), 0, 24))[0] == 0  # shifts behind the layers are not read

    def run():
        res = [(what, size(8, params(**kw)), lib.oth_last_error(), word) for what, kw, word in BAD_PARAMS]
        res += [("board_size = %d" % n, size(n, params()), lib.oth_last_error(), b"board_size") for n in (3, 17)]
        res.append(("NULL params", size(8, None), lib.oth_last_error(), b"params"))
        res.append(("NULL bytes", (lib.oth_net_blob_bytes(8, ctypes.byref(params()), None), 0), lib.oth_last_error(),
                    b"bytes"))
        return res

    for what, (rc, b), msg, word in on_a_thread(run):
        assert rc == -1 and b == 0 and msg and word in msg, (what, msg)


@pytest.mark.parametrize("i", (1, 2, 5, 8), ids=lambda i: nc.IDS[i])
def test_pack_is_the_host_builds(lib, i):
    c = nc.case(i)
    w, b = nc.flat_weights(c)
    size = nc.blob_bytes(c.n, c.L, c.H)
    p = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    whole = np.full(size + 64 + 16, 0xA5, np.uint8)
    at = (-whole.ctypes.data) % 16
    blob = whole[at:at + size]
    assert lib.oth_net_pack(c.n, ctypes.byref(p), ptr(w), ptr(b), ptr(blob), size) == 0
    assert (whole[:at] == 0xA5).all() and (whole[at + size:] == 0xA5).all()
    want = np.zeros(size, np.uint8)
    hp = host_params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    assert load_hostlib().host_net_pack(c.n, ctypes.byref(hp), ptr(w), ptr(b), ptr(want)) == 0
    assert (blob == want).all()


def test_argument_checks_without_gpu(lib):
    c = nc.case(0)
    w, b = nc.flat_weights(c)
    size = nc.blob_bytes(8, 2, 128)
    whole = np.zeros(size + 32, np.uint8)
    at = (-whole.ctypes.data) % 16
    blob = ctypes.c_void_p(whole.ctypes.data + at)
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    good = params()

    def ref(p):
        return None if p is None else ctypes.byref(p)

    def pack(n=8, p=good, w_=ptr(w), b_=ptr(b), blob_=blob, nbytes=size):
        return lib.oth_net_pack, (n, ref(p), w_, b_, blob_, nbytes)

    def ev(n=8, R=4, p=good, blob_=blob, nbytes=1 << 40, boards=arr, meta=arr, legal=arr, priors=arr, values=arr):
        return lib.oth_net_eval, (n, R, ref(p), blob_, nbytes, boards, meta, legal, priors, values, None, None)

    cases = []
    for name, call in (("pack", pack), ("eval", ev)):
        cases += [(name + ": " + what, call(p=params(**kw)), word) for what, kw, word in BAD_PARAMS]
        cases += [(name + ": NULL params", call(p=None), b"params"),
                  (name + ": board_size = 3", call(n=3), b"board_size"),
                  (name + ": board_size = 17", call(n=17), b"board_size"),
                  (name + ": NULL blob", call(blob_=None), b"blob"),
                  (name + ": misaligned blob", call(blob_=ctypes.c_void_p(blob.value + 8)), b"aligned"),
                  (name + ": short blob", call(nbytes=size - 1), b"blob_bytes")]
    cases += [("pack: NULL w", pack(w_=None), b"NULL"), ("pack: NULL b", pack(b_=None), b"NULL"),
              ("eval: NULL boards", ev(boards=None), b"boards"), ("eval: NULL meta", ev(meta=None), b"meta"),
              ("eval: NULL legal", ev(legal=None), b"legal"), ("eval: NULL priors", ev(priors=None), b"priors"),
              ("eval: NULL values", ev(values=None), b"values"), ("eval: n_rows = -1", ev(R=-1), b"n_rows"),
              ("eval: n_rows = 2^24 + 1", ev(R=(1 << 24) + 1), b"n_rows")]

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert msg and word in msg, (what, msg)
    assert list(out) == [0] * 64 and not whole.any()  # nothing was written
    # a bias out of range, found by the pack step before anything is written
    w8 = np.zeros(128 * 192 + 128 * 128 + 65 * 128, np.int8)
    for at_, v in ((0, (1 << 30) + 1), (2 * 128 + 64, -(1 << 30) - 1)):
        b8 = np.zeros(2 * 128 + 65, np.int32)
        b8[at_] = v
        fn, args = pack(w_=ptr(w8), b_=ptr(b8))
        assert fn(*args) == -1 and not whole.any()
    # no rows: nothing to launch, and no GPU needed to say so
    fn, args = ev(R=0)
    assert fn(*args) == 0


def test_python_surface():
    import gymothelloenv_amd as g
    from gymothelloenv_amd import net

    assert g.DeviceNet is net.DeviceNet and g.MLPPolicyValue is net.MLPPolicyValue and g.net_features is net.net_features
    assert net.DeviceNet.quantized is True
    names = list(inspect.signature(net.DeviceNet.__init__).parameters)[1:]
    assert names == ["board_size", "weights", "biases", "shifts", "policy_shift", "value_shift", "device"]
    assert list(inspect.signature(net.DeviceNet.evaluate).parameters)[1:] == ["boards", "meta", "legal", "logits"]
    assert list(inspect.signature(net.MLPPolicyValue.__init__).parameters)[1:4] == ["board_size", "hidden", "layers"]
    assert list(inspect.signature(net.net_features).parameters) == ["boards", "meta", "legal", "board_size"]
