"""The convolutional network's core (csrc/cnet.hpp: the packed layout, the pack step
and the row evaluation that reads the bytes the device kernel reads, compiled for the
host with g++: tests/host/cnet_host.cpp) against the numpy and Python integers of
tests/cnet_ref.py on every case of tests/cnet_cases.py, with guard words behind every
buffer.  Every comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cnet_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "cnet_host.cpp")
LIB = os.path.join(HERE, "host", "libcnet_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("cnet.hpp", "net.hpp", "bitboard.hpp")]
GUARD = 64  # bytes or elements behind a buffer that no call may touch


class Params(ctypes.Structure):
    _fields_ = [("channels", ctypes.c_int32), ("blocks", ctypes.c_int32), ("shift_stem", ctypes.c_int32),
                ("shift", ctypes.c_int32 * 16), ("shift_head", ctypes.c_int32), ("policy_shift", ctypes.c_int32),
                ("value_shift", ctypes.c_int32)]


def params(C, B, shift_stem, shifts, shift_head, policy_shift, value_shift):
    sh = list(shifts) + [0] * (16 - len(shifts))
    return Params(C, B, shift_stem, (ctypes.c_int32 * 16)(*sh), shift_head, policy_shift, value_shift)


def case_params(c, **kw):
    d = dict(C=c.C, B=c.B, shift_stem=c.shift_stem, shifts=c.shifts, shift_head=c.shift_head,
             policy_shift=c.policy_shift, value_shift=c.value_shift)
    d.update(kw)
    return params(**d)


def load_hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    for name in ("host_cnet_blob_bytes", "host_cnet_weights", "host_cnet_biases"):
        getattr(L, name).argtypes = [I, P]
        getattr(L, name).restype = ctypes.c_uint64
    L.host_cnet_check.argtypes = [I, P, ctypes.c_char_p, I]
    L.host_cnet_check.restype = None
    L.host_cnet_pack.argtypes = [I, P, P, P, P]
    L.host_cnet_eval.argtypes = [I, P, I, P, P, P, P, P, P, P]
    return L


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def guarded(shape, dtype, fill=7):
    """(the whole buffer, the view a call gets): GUARD elements of `fill` behind the view."""
    count = int(np.prod(shape))
    whole = np.full(count + GUARD, fill, dtype=dtype)
    return whole, whole[:count].reshape(shape)


def packed(L, c, p):
    """A case's blob, packed by the host build into a buffer of exactly the reported size."""
    size = int(L.host_cnet_blob_bytes(c.n, ctypes.byref(p)))
    assert size == cc.blob_bytes(c.n, c.B, c.C) and size % 16 == 0
    whole, blob = guarded((size,), np.uint8, 0xA5)
    w, b = cc.flat_weights(c)
    assert (w.size, b.size) == (L.host_cnet_weights(c.n, ctypes.byref(p)), L.host_cnet_biases(c.n, ctypes.byref(p)))
    assert L.host_cnet_pack(c.n, ctypes.byref(p), ptr(w), ptr(b), ptr(blob)) == 0
    assert (whole[size:] == 0xA5).all()
    return blob


@pytest.mark.parametrize("i", range(len(cc.TABLE)), ids=cc.IDS)
def test_exact_against_the_reference(hostlib, i):
    c = cc.case(i)
    p = case_params(c)
    blob = packed(hostlib, c, p)
    pw, priors = guarded((c.R, c.nn), np.int32)
    vw, values = guarded((c.R,), np.int32)
    lw, logits = guarded((c.R, c.nn + 1), np.int32)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    assert hostlib.host_cnet_eval(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), ptr(priors),
                                  ptr(values), ptr(logits)) == 0
    np.testing.assert_array_equal(logits, c.logits)
    np.testing.assert_array_equal(values, c.values)
    np.testing.assert_array_equal(priors, c.priors)
    for whole, view in ((pw, priors), (vw, values), (lw, logits)):
        assert (whole[view.size:] == 7).all()
    if c.R <= 20:  # without the logits: the same priors and values
        p2, v2 = np.full_like(priors, 7), np.full_like(values, 7)
        assert hostlib.host_cnet_eval(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), ptr(p2),
                                      ptr(v2), None) == 0
        assert (p2 == priors).all() and (v2 == values).all()


def test_the_blob_begins_with_its_own_tags(hostlib):
    """Two tags whose prefixes are not oth_net's ("net", "ws"), then the block shifts; the parts are 16-byte aligned
    and hold no addresses: packing twice gives the same bytes."""
    c = cc.case(2)
    p = case_params(c)
    blob = packed(hostlib, c, p)
    tags = blob[:16].view(np.uint64)
    assert int(tags[0]) >> 32 == 0x636e6574 and int(tags[1]) >> 32 == 0x63736866
    assert int(tags[0]) >> 40 != 0x6e6574 and int(tags[1]) >> 48 != 0x7773
    assert blob[16:32].tolist() == list(c.shifts) + [0] * (16 - 2 * c.B)
    assert (packed(hostlib, c, p) == blob).all()


def test_high_bits_and_meta_bits_are_not_read(hostlib):
    c = cc.case(5)  # N = 10: 100 squares, 28 bits of the second word off the board
    p = case_params(c)
    blob = packed(hostlib, c, p)
    off = ~np.uint64(0) << np.uint64(c.nn - 64)
    boards, legal = c.boards.copy(), c.legal.copy()
    boards[:, 1] ^= off
    boards[:, 3] ^= off
    legal[:, 1] ^= off
    meta = c.meta ^ np.uint16(0xFFFE)
    order = np.arange(c.R)[::-1].copy()
    b2, m2, l2 = boards[order].copy(), meta[order].copy(), legal[order].copy()
    priors, values = np.full((c.R, c.nn), 7, np.int32), np.full(c.R, 7, np.int32)
    assert hostlib.host_cnet_eval(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(b2), ptr(m2), ptr(l2), ptr(priors),
                                  ptr(values), None) == 0
    np.testing.assert_array_equal(priors, c.priors[order])
    np.testing.assert_array_equal(values, c.values[order])


def test_another_geometry_or_other_shifts_write_nothing(hostlib):
    c = cc.case(1)
    p = case_params(c)
    blob = packed(hostlib, c, p)
    priors, values = np.full((c.R, c.nn), 7, np.int32), np.full(c.R, 7, np.int32)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    others = [case_params(c, policy_shift=c.policy_shift + 1), case_params(c, value_shift=c.value_shift + 1),
              case_params(c, shift_stem=c.shift_stem + 1), case_params(c, shift_head=c.shift_head + 1),
              case_params(c, shifts=[c.shifts[0], c.shifts[1] + 1]), case_params(c, C=128),
              case_params(c, B=2, shifts=list(c.shifts) + [0, 0])]
    for other in others:
        assert hostlib.host_cnet_eval(c.n, ctypes.byref(other), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal),
                                      ptr(priors), ptr(values), None) == 2
        assert (priors == 7).all() and (values == 7).all()
    # an MLP's tags are no conv net's
    mlp = blob.copy()
    mlp[:16] = np.array([0x6e65740000000000 | c.n << 32 | 1 << 16 | 64, 0x7773000000000000], np.uint64).view(np.uint8)
    assert hostlib.host_cnet_eval(c.n, ctypes.byref(p), c.R, ptr(mlp), ptr(boards), ptr(meta), ptr(legal), ptr(priors),
                                  ptr(values), None) == 2
    assert (priors == 7).all() and (values == 7).all()


CHECKS = [(dict(), 3, b"board_size must be in [4, 16]"), (dict(), 17, b"board_size must be in [4, 16]"),
          (dict(C=32), 8, b"channels must be 64 or 128"), (dict(C=96), 8, b"channels must be 64 or 128"),
          (dict(C=256), 8, b"channels must be 64 or 128"), (dict(B=0, shifts=[]), 8, b"blocks must be in [1, 8]"),
          (dict(B=9, shifts=[0] * 16), 8, b"blocks must be in [1, 8]"),
          (dict(shift_stem=25), 8, b"shift_stem must be in [0, 24]"), (dict(shift_stem=-1), 8, b"shift_stem must be in [0, 24]"),
          (dict(shifts=[0, 25]), 8, b"every shift must be in [0, 24]"), (dict(shifts=[-1, 0]), 8, b"every shift must be in [0, 24]"),
          (dict(shift_head=25), 8, b"shift_head must be in [0, 24]"), (dict(shift_head=-1), 8, b"shift_head must be in [0, 24]"),
          (dict(policy_shift=25), 8, b"policy_shift must be in [0, 24]"),
          (dict(policy_shift=-1), 8, b"policy_shift must be in [0, 24]"),
          (dict(value_shift=25), 8, b"value_shift must be in [0, 24]"), (dict(value_shift=-1), 8, b"value_shift must be in [0, 24]")]


def test_every_message_of_the_check(hostlib):
    base = dict(C=64, B=1, shift_stem=0, shifts=[0, 0], shift_head=0, policy_shift=0, value_shift=0)
    msg = ctypes.create_string_buffer(128)
    hostlib.host_cnet_check(8, None, msg, 128)
    assert msg.value == b"params is NULL"
    seen = {msg.value}
    for kw, n, want in CHECKS:
        p = params(**dict(base, **kw))
        hostlib.host_cnet_check(n, ctypes.byref(p), msg, 128)
        assert msg.value == want, (kw, n)
        assert hostlib.host_cnet_blob_bytes(n, ctypes.byref(p)) == 0
        seen.add(msg.value)
    assert len(seen) == 9  # every message cnet_check has
    good = params(**dict(base, shifts=[0, 0, 99, -5]))  # shifts behind the blocks are not read
    hostlib.host_cnet_check(8, ctypes.byref(good), msg, 128)
    assert msg.value == b"" and hostlib.host_cnet_blob_bytes(8, ctypes.byref(good)) == cc.blob_bytes(8, 1, 64)


def test_pack_rejects_a_bias_out_of_range(hostlib):
    c = cc.case(0)
    w, b = cc.flat_weights(c)
    p = case_params(c)
    blob = np.zeros(cc.blob_bytes(c.n, c.B, c.C), np.uint8)
    for at, v in ((0, 2 ** 30 + 1), (b.size - 1, -2 ** 30 - 1), (c.C, 2 ** 31 - 1)):
        b2 = b.copy()
        b2[at] = v
        assert hostlib.host_cnet_pack(c.n, ctypes.byref(p), ptr(w), ptr(b2), ptr(blob)) == 2
        assert not blob.any()
    assert hostlib.host_cnet_pack(c.n, ctypes.byref(p), ptr(w), ptr(b), ptr(blob)) == 0
