"""The convolutional network's C ABI without a GPU: oth_cnet_blob_bytes and
oth_cnet_pack, which run on the host, and every argument check of oth_cnet_eval (with
nothing launched), in the manner of tests/test_net_capi_cpu.py."""
import ctypes
import threading

import numpy as np
import pytest

import cnet_cases as cc
from test_cnet_host import case_params as host_case_params, load_hostlib, ptr


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


def params(C=64, B=2, shift_stem=1, shifts=(5, 6, 7, 8), shift_head=9, policy_shift=8, value_shift=3):
    from gymothelloenv_amd import _lib as L_
    sh = list(shifts) + [0] * (16 - len(shifts))
    return L_.OthCnetParams(C, B, shift_stem, (ctypes.c_int32 * 16)(*sh), shift_head, policy_shift, value_shift)


BAD_PARAMS = [("channels = 32", dict(C=32), b"channels"), ("channels = 96", dict(C=96), b"channels"),
              ("channels = 256", dict(C=256), b"channels"), ("blocks = 0", dict(B=0), b"blocks"),
              ("blocks = 9", dict(B=9, shifts=(0,) * 16), b"blocks"), ("shift_stem = 25", dict(shift_stem=25), b"shift_stem"),
              ("shift_stem = -1", dict(shift_stem=-1), b"shift_stem"), ("shift = 25", dict(shifts=(5, 6, 7, 25)), b"shift"),
              ("shift = -1", dict(shifts=(-1, 6, 7, 8)), b"shift"), ("shift_head = 25", dict(shift_head=25), b"shift_head"),
              ("shift_head = -1", dict(shift_head=-1), b"shift_head"),
              ("policy_shift = 25", dict(policy_shift=25), b"policy_shift"),
              ("policy_shift = -1", dict(policy_shift=-1), b"policy_shift"),
              ("value_shift = 25", dict(value_shift=25), b"value_shift"),
              ("value_shift = -1", dict(value_shift=-1), b"value_shift")]


def test_blob_bytes(lib):
    from gymothelloenv_amd import _lib as L
    assert L.OTH_CNET_MAX_BLOCKS == 8
    S = L.OthCnetParams
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [
        ("channels", 0), ("blocks", 4), ("shift_stem", 8), ("shift", 12), ("shift_head", 76), ("policy_shift", 80),
        ("value_shift", 84)]
    assert ctypes.sizeof(S) == 88

    def size(n, p):
        b = ctypes.c_uint64(0)
        return lib.oth_cnet_blob_bytes(n, None if p is None else ctypes.byref(p), ctypes.byref(b)), b.value

    for n in range(4, 17):
        for B in (1, 3, 8):
            for C in (64, 128):
                assert size(n, params(C, B, shifts=(3,) * (2 * B))) == (0, cc.blob_bytes(n, B, C)), (n, B, C)
    assert size(8, params(64, 1, shifts=(24, 0, 99, -5)))[0] == 0  # shifts behind the blocks are not read

    def run():
        res = [(what, size(8, params(**kw)), lib.oth_last_error(), word) for what, kw, word in BAD_PARAMS]
        res += [("board_size = %d" % n, size(n, params()), lib.oth_last_error(), b"board_size") for n in (3, 17)]
        res.append(("NULL params", size(8, None), lib.oth_last_error(), b"params"))
        res.append(("NULL bytes", (lib.oth_cnet_blob_bytes(8, ctypes.byref(params()), None), 0), lib.oth_last_error(),
                    b"bytes"))
        return res

    for what, (rc, b), msg, word in on_a_thread(run):
        assert rc == -1 and b == 0 and msg and word in msg, (what, msg)


@pytest.mark.parametrize("i", (0, 2, 5), ids=lambda i: cc.IDS[i])
def test_pack_is_the_host_builds(lib, i):
    from gymothelloenv_amd.cnet import DeviceConvNet
    c = cc.case(i)
    w, b = cc.flat_weights(c)
    size = cc.blob_bytes(c.n, c.B, c.C)
    p, fw, fb = DeviceConvNet.flatten(c.n, *cc.net_args(c))  # the Python surface's flat order is the header's
    np.testing.assert_array_equal(fw.numpy(), w)
    np.testing.assert_array_equal(fb.numpy(), b)
    whole = np.full(size + 64 + 16, 0xA5, np.uint8)
    at = (-whole.ctypes.data) % 16
    blob = whole[at:at + size]
    assert lib.oth_cnet_pack(c.n, ctypes.byref(p), ptr(w), ptr(b), ptr(blob), size) == 0
    assert (whole[:at] == 0xA5).all() and (whole[at + size:] == 0xA5).all()
    want = np.zeros(size, np.uint8)
    hp = host_case_params(c)
    assert load_hostlib().host_cnet_pack(c.n, ctypes.byref(hp), ptr(w), ptr(b), ptr(want)) == 0
    assert (blob == want).all()


def test_argument_checks_without_gpu(lib):
    n, C, B = 8, 64, 2
    size = cc.blob_bytes(n, B, C)
    w = np.zeros(C * 27 + 2 * B * C * C * 9 + 16 * C * 9 + 64 * 15, np.int8)
    b = np.zeros(C * (1 + 2 * B) + 16 + 1, np.int32)
    whole = np.zeros(size + 32, np.uint8)
    at = (-whole.ctypes.data) % 16
    blob = ctypes.c_void_p(whole.ctypes.data + at)
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    good = params()

    def ref(p):
        return None if p is None else ctypes.byref(p)

    def pack(n=n, p=good, w_=ptr(w), b_=ptr(b), blob_=blob, nbytes=size):
        return lib.oth_cnet_pack, (n, ref(p), w_, b_, blob_, nbytes)

    def ev(n=n, R=4, p=good, blob_=blob, nbytes=1 << 40, boards=arr, meta=arr, legal=arr, priors=arr, values=arr):
        return lib.oth_cnet_eval, (n, R, ref(p), blob_, nbytes, boards, meta, legal, priors, values, None, None)

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
    for at_, v in ((0, (1 << 30) + 1), (b.size - 1, -(1 << 30) - 1)):
        b2 = b.copy()
        b2[at_] = v
        fn, args = pack(b_=ptr(b2))
        assert fn(*args) == -1 and not whole.any()
    # no rows: nothing to launch, and no GPU needed to say so
    fn, args = ev(R=0)
    assert fn(*args) == 0
    fn, args = pack()
    assert fn(*args) == 0 and whole[at:at + 32].any() and not whole[at + size:].any()
